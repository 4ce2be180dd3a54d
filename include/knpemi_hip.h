/* libknpemi_hip.so -- C ABI of the MI355X-native DG assemble-and-solve path of knpemidg.Solver.
 *
 * This is the drop-in seam that replaces, inside adajel/KNP-EMI-DG's `Solver`,
 *   - UFL form assembly      dolfin.assemble(a_emi|L_emi|B_emi|A_knp|L_knp)   src/knpemidg/solver.py:452-453,477-479,710,730-731
 *   - the PETSc matrix build  as_backend_type(...).mat()                      src/knpemidg/solver.py:458-460,482-484,711-712,734-735
 *   - the PETSc KSP solves    ksp.solve (cg / gmres + hypre)                  src/knpemidg/solver.py:509,755,771
 *   - the step-III projections pcws_constant_project / project               src/knpemidg/solver.py:808-845, utils.py:100-124
 * with matrix-free HIP kernels.  All functions are extern "C", take plain pointers and sizes,
 * return 0 on success and a negative status on failure (message: knp_last_error).  The caller
 * owns every host buffer; the context owns every device buffer.  One host thread per context,
 * one HIP stream per context; calls are synchronous with respect to the host unless noted.
 *
 * DoF layout (build-defined): scalar DG-p field  dof(c, j) = c*nd + j ;
 * species-major for the KNP unknown [k][c][j] ; facet fields one value per facet.
 * Cells hold ASCENDING vertex ids; local facet i is opposite local vertex i.
 */
#ifndef KNPEMI_HIP_H
#define KNPEMI_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct knp_ctx knp_ctx;

/* device-resident fields addressable through knp_upload / knp_download / knp_*_apply */
enum knp_field {
    KNP_F_PHI = 0,       /* potential phi                    [nc*nd]          Solver.phi          solver.py:165 */
    KNP_F_C = 1,         /* solved concentrations c          [n_sys][nc*nd]   Solver.c / c_prev_k solver.py:172-176 */
    KNP_F_C_PREV = 2,    /* c at previous time level         [n_sys][nc*nd]   Solver.c_prev_n     solver.py:174 */
    KNP_F_C_ELIM = 3,    /* eliminated ion                   [nc*nd]          ion_list[-1]['c']   solver.py:191 */
    KNP_F_PHI_M = 4,     /* membrane potential on facets     [nf]             phi_M_prev_PDE      solver.py:214 */
    KNP_F_I_CH = 5,      /* channel currents per ion         [n_ions][nf]     mem_models[..]['I_ch_k'] solver.py:251-259 */
    KNP_F_E = 6,         /* Nernst potentials per ion        [n_ions][nf]     ion['E']            solver.py:299-300 */
    KNP_F_KAPPA = 7,     /* kappa (derived)                  [nc*nd]          solver.py:306 */
    KNP_F_DNPHI = 8,     /* grad(phi).n per local facet      [nc*nd]          (derived, feeds solver.py:583,593) */
    KNP_F_B_EMI = 9,     /* assembled L_emi                  [nc*nd]          bb_emi              solver.py:478 */
    KNP_F_B_KNP = 10,    /* assembled L_knp                  [n_sys][nc*nd]   bb_knp              solver.py:731 */
    KNP_F_X = 11,        /* scratch vector                   [n_sys][nc*nd] */
    KNP_F_Y = 12,        /* scratch vector                   [n_sys][nc*nd] */
    KNP_F_FACET_TMP = 13,/* scratch facet fields             [KNP_FACET_TMP_SLOTS][nf]   results of pcws_constant_project */
    KNP_F_COUNT = 14
};

/* ---- context -------------------------------------------------------------------------------
 * Uploads the mesh and derives the per-(cell, local facet) neighbour / flag tables and the
 * membrane facet table.  Replaces Solver.setup_domain + interface_normal + subdomain_marking_foo
 * (solver.py:85-121, utils.py:44-85).
 *  cells        i32[nc][dim+1] vertex ids, local order = ascending ids of the caller's mesh (ids may then be
 *               relabelled for storage locality); cells [0,nc_owned) are owned, the rest are ghosts
 *  cell_tags    u32[nc]         subdomain tags (0 = ECS)
 *  facet_cells  i32[nf][2]      cells sharing each facet, -1 = none
 *  facet_local  i8 [nf][2]      local facet index within those cells
 *  facet_tags   u32[nf]         0 = ordinary interior facet (solver.py:60), membrane tags listed in membrane_tags
 */
int knp_ctx_create(knp_ctx** out, int device, int dim, int degree, int n_ions,
                   int64_t nv, int64_t nc, int64_t nc_owned, int64_t nf,
                   const double* coords, const int32_t* cells, const uint32_t* cell_tags,
                   const int32_t* facet_cells, const int8_t* facet_local, const uint32_t* facet_tags,
                   int n_membrane_tags, const uint32_t* membrane_tags);
void knp_ctx_destroy(knp_ctx* ctx);
const char* knp_last_error(knp_ctx* ctx);

/* Physical parameters (Solver.setup_parameters, solver.py:124-154; tau: solver.py:109-111).
 *  z[n_ions], D[n_ions][nc] (make_global, solver.py:1244-1258), rho[nc], fsrc[n_sys][nc] or NULL
 *  (ion['f_source'] on dx(0), solver.py:599), splitting: 1 = splitting scheme, 0 = original Robin
 *  data (solver.py:332-337, 614-622), 2 = manufactured-solution mode (knp_set_mms). */
int knp_set_params(knp_ctx* ctx, double C_M, double dt, double F, double R, double T, double C_phi,
                   double tau_emi, double tau_knp, const double* z, const double* D, const double* rho,
                   const double* fsrc, int splitting);

/* Optional geometry classes for (block-)structured meshes: cells with identical shape and neighbour-apex
 * positions share one 36-double record {vol, G upper triangle (10), per facet: L[4], sqrt(G_ii), 2/(h+h')}; the
 * operator applies then read no coordinates at all.  ncls = 0 switches back to the coordinate path. */
int knp_set_geometry_classes(knp_ctx* ctx, int ncls, const uint16_t* cls, const double* table);

/* Manufactured-solution mode (Solver(mms=...), solver.py:349-374, 632-657): splitting = 2 in knp_set_params selects
 * it.  C[n_sys][nc] are the DG0 coupling coefficients ion['C']; extra_emi[nc*nd] / extra_knp[n_sys][nc*nd] are the
 * solution-independent data terms (volume sources, Robin and flux-continuity data, Neumann data) integrated on the
 * host and added to L_emi / L_knp; the solution-dependent term -jump(phi) jump(C v) is evaluated on the device.
 * Every call replaces all three tables (a null pointer drops that table).  While splitting == 2 a null C is refused: the
 * call returns -1 with a message in knp_last_error and leaves the tables of the previous call in place. */
int knp_set_mms(knp_ctx* ctx, const double* C, const double* extra_emi, const double* extra_knp);

/* Ion sources that are not constants (ion['f_source'] is any UFL coefficient in the reference, solver.py:599; e.g. the box- and
 * time-window Expression of examples/local-astrocyte-depolarization/run_tortuosity.py:180-200): src[n_sys][nc*nd] = the load
 * vector int f_k v dx(0) integrated by the caller, added to L_knp by knp_knp_rhs; null clears.  Constant sources travel as
 * fsrc[n_sys][nc] of knp_set_params. */
int knp_set_source(knp_ctx* ctx, const double* src);

/* Ion sources evaluated on the device (knpemidg.Expression): a scalar C++ expression of x and named parameters, wrapped by
 * knpemidg/expression.py into a translation unit around csrc/source_rtc.hpp and compiled with knp_ode_rtc_compile.  Its kernel
 * writes, for every ECS cell of the context (tag 0, owned and ghost -- the `dx(0)` of solver.py:599) and local basis function a,
 * vol * sum_q w_q f(x_q) B[q][a] into the species' row of the buffer of knp_set_source: one lane per cell, fixed summation order,
 * no atomics (same bits on every run), overwriting (a repeated evaluation changes nothing).
 *  knp_source_set_rule: the rule the kernels integrate with, once per context before the first registration: bary[nq][dim+1],
 *                       w[nq] (sums to 1), B[nq][nd] basis values at the points; 1 <= nq <= 4096.  The caller tabulates them, so
 *                       host and device use the same numbers
 *  knp_source_register: loads the code object on the context's device as the source of `species` (replacing an earlier one; the
 *                       modules are unloaded with the context).  The first call builds the list of ECS cells; the buffer is
 *                       allocated zero-filled if absent.  -1 in manufactured-solution mode (splitting == 2), for a species outside
 *                       [0, n_sys), for n_params outside 0..32 and without a rule
 *  knp_source_eval    : enqueues the species' kernel on the context's stream with params[n_params] BY VALUE in the kernel
 *                       arguments: no copy to the device, no synchronisation (knp_host_round_trips does not move).  An empty cell
 *                       list launches nothing.  With knp_set_source in the same step, call that first: rows of device sources are
 *                       then overwritten, rows of host-integrated sources survive
 *  knp_source_clear   : drops the species' kernel and zeroes its row
 *  knp_source_cells   : length of the ECS cell list (-1 before the first registration)
 *  knp_source_download: the whole buffer, out[n_sys][nc*nd] in device cell order, for tests (waits for the stream); 1 and `out`
 *                       untouched when the context has no buffer */
int knp_source_set_rule(knp_ctx* ctx, int nq, const double* bary, const double* w, const double* B);
int knp_source_register(knp_ctx* ctx, int species, const void* code, size_t size, const char* kernel_name, int n_params);
int knp_source_eval(knp_ctx* ctx, int species, const double* params, int n_params);
int knp_source_clear(knp_ctx* ctx, int species);
int64_t knp_source_cells(knp_ctx* ctx);
int knp_source_download(knp_ctx* ctx, double* out);

/* Ion sources that read the solution, on any subdomain (knpemidg.FieldExpression): as knp_source_register, with two additions.
 *  - field_ids[n_fields], distinct, 0 <= n_fields <= 9: 0 is phi, 1 + i is ion i of the ion list -- i < n_sys is row i of
 *    KNP_F_C_PREV, i == n_sys is KNP_F_C_ELIM (the convention of knp_grid_create).  The kernel's functor receives their values at
 *    the quadrature point, u(x_q) = sum_a U[a] B[q][a], in this order.  The pointers are looked up at every knp_source_eval, so
 *    an evaluation in front of a KNP solve sees the concentrations of the previous time level (the same in every Picard iteration
 *    of a step) and the phi of the EMI solve just done.
 *  - tags[n_tags], n_tags >= 1: the kernel integrates over its OWN cell list, the cells of the context (owned and ghost, ascending
 *    device order) whose tag is one of them.  No such cell: the row stays zero and an evaluation launches nothing.  The shared ECS
 *    list of knp_source_register and knp_source_cells are untouched by this call.
 * Registering over an existing source of the species, of either kind, first zeroes the species' row on the stream: cells that
 * left the selection hold exact zeros.  knp_source_eval / _clear serve both kinds; knp_source_clear and knp_ctx_destroy free the
 * kernel's list.  -1 for everything knp_source_register refuses, for a field id outside [0, n_ions] or listed twice, for n_fields
 * above 9 and for n_tags < 1. */
int knp_source_register_fields(knp_ctx* ctx, int species, const void* code, size_t size, const char* kernel_name, int n_params,
                               int n_fields, const int* field_ids, int n_tags, const int* tags);

/* DG-p path (degree 2): reference-basis tabulation of one integral class.  The operator applies are matrix-free and need
 * no tabulation (csrc/apply_p2.hip); the right-hand sides, facet averages and Nernst projections of step III (the device
 * analogue of assemble(L_emi / L_knp), solver.py:477-479, 730-731, and of pcws_constant_project, utils.py:100-124) are
 * integrated by numerical quadrature from these tables; the rules and the basis tabulated at their points come from the host
 * (knpemidg/dgtab.py).
 *  w[nq] weights summing to 1;  B[nloc][nq][nd] basis values;  dB[nloc][nq][nd][dim+1] derivatives with respect to
 *  the barycentric coordinates;  nloc = 1 for cell rules, dim+1 for facet rules (one tabulation per local facet, all
 *  with the same facet points: facet vertex m <-> cell vertex m + (m >= local facet index)).
 * Local dof order of a P2 cell: the dim+1 vertices, then the edge midpoints (a,b), a<b, lexicographic. */
enum knp_tab_slot {
    KNP_TAB_CELL_STIFF = 0,     /* dx of a_emi / a_knp                  degree max(2, 3p-2, 2p)  solver.py:318, 550-556 */
    KNP_TAB_CELL_RHS_EMI = 1,   /* dx of L_emi                          degree max(1, 2p-2)      solver.py:309-310 */
    KNP_TAB_CELL_MASS = 2,      /* dx of L_knp                          degree 2p                solver.py:597-599 */
    KNP_TAB_FACET_EMI = 3,      /* dS(0) of a_emi                       degree 3p                solver.py:321-328 */
    KNP_TAB_FACET_MEM = 4,      /* dS(membrane) of a_emi                degree 2p                solver.py:344 */
    KNP_TAB_FACET_KNP = 5,      /* dS(0) of a_knp                       degree max(2, 3p-1)      solver.py:586-594 */
    KNP_TAB_FACET_RHS_EMI = 6,  /* dS(0) of L_emi                       degree max(1, 2p-1)      solver.py:330 */
    KNP_TAB_FACET_MEM_LIN = 7,  /* dS(membrane) of L_emi                degree max(1, 2p-1)      solver.py:332-344 */
    KNP_TAB_FACET_MEM_KNP = 8,  /* dS(membrane) of L_knp                degree 5p                solver.py:603-629 */
    KNP_TAB_FACET_AVG = 9,      /* facet averages (phi_M, traces)       degree max(1, p)         utils.py:100-124 */
    KNP_TAB_FACET_NERNST = 10   /* ln(c_e/c_i)                          degree 2p+2              solver.py:827-828 */
};
int knp_set_tabulation(knp_ctx* ctx, int slot, int nloc, int nq, const double* w, const double* B, const double* dB);

int64_t knp_field_size(knp_ctx* ctx, int field);
int knp_upload(knp_ctx* ctx, int field, const double* src, int64_t offset, int64_t count);
int knp_download(knp_ctx* ctx, int field, double* dst, int64_t offset, int64_t count);
int knp_copy_field(knp_ctx* ctx, int dst_field, int src_field);

/* Inspection of the connectivity tables the library derives in knp_ctx_create from the raw cell / facet / tag arrays -- the
 * device counterpart of interface_normal / plus / minus (utils.py:61-98) and of the dS / membrane facet classification by tag
 * (solver.py:113-121).  `north_star` asks for bit-exact DoF / connectivity indexing: the parity tests read these tables back and
 * compare them entry for entry with the oracle's independently derived ones (tests/test_gpu_tables.py).  All tables are in DEVICE
 * cell order (the order of the `cells` argument of knp_ctx_create); facet ids are the caller's.
 *  knp_debug_table_size: number of BYTES of table `which`, < 0 if unknown
 *  knp_debug_table     : copies the table into out[nbytes]; nbytes must equal knp_debug_table_size */
enum knp_debug_table_id {
    KNP_DT_CELLS = 0,   /* int32  [nc][dim+1]  cell -> vertex (storage ids)                                                   */
    KNP_DT_NBR = 1,     /* int32  [nc][dim+1]  cell behind local facet i (opposite vertex i), -1 on the boundary              */
    KNP_DT_FLAG = 2,    /* uint32 [nc]         dim+1 flag bytes: bits 0-1 local facet index in the neighbour, bits 2-3 kind
                                               (0 SIPG, 1 membrane, 2 exterior, 3 inactive), bit 4 this cell is the `plus` side */
    KNP_DT_CFACET = 3,  /* int32  [nc][dim+1]  facet id behind local facet i                                                  */
    KNP_DT_MF = 4,      /* int32  [nmf][6]     membrane facets: plus cell, minus cell, their local facet indices, facet id,
                                               1 if a side is an owned cell                                                     */
    KNP_DT_HB_SRC = 5,  /* int32  [nblk][hs]   halo- / ring-staged applies: per 256-cell block, 4 * cell + local facet of every
                                               coupled (SIPG or membrane) neighbour outside the block, in (cell, facet) order, -1 padded (0 bytes if unused) */
    KNP_DT_HB_LOC = 6,  /* uint16 [nc_owned][4] LDS entry of the neighbour behind facet i: < 256 in-block, else 256 + list position */
    KNP_DT_META = 7,    /* int64  [8]          nc, nc_owned, nf, nmf, hb_stride, hb_long0, n_interior, dim                     */
    /* The per-block tables of the unstructured ring-staged applies (3D P1 meshes without geometry classes, csrc/apply_ring_u.hip).
     * Asking for one builds them as the first apply would; every one has 0 bytes when the context has no usable unstructured ring
     * (classes present, first block over a limit, KNP_APPLY_RING_U=0, ...).  nblk = ceil(nc_owned / 256).  Blocks [0, long0) fit the
     * staging limits (320 list entries, 256 vertices); rows of later blocks and of their cells are unspecified. */
    KNP_DT_RU_META = 8,   /* int64  [4]          long0, hs (longest list of a covered block, at least 1), nblk, covered cells
                                                 min(long0 * 256, nc_owned): what apply variant 10 runs, the rest goes to the tail kernel */
    KNP_DT_RU_HB_SRC = 9, /* int32  [nblk][320]  per block, 4 * cell + the neighbour's local facet of every coupled (SIPG or membrane)
                                                 neighbour that is outside the block OR not owned, in (cell, facet) order, -1 padded   */
    KNP_DT_RU_HB_LOC = 10,/* uint16 [nc_owned][4] LDS entry of the neighbour behind facet i: < 256 in-block, else 256 + list position
                                                 (0 where the facet couples nothing)                                                  */
    KNP_DT_RU_VB_SRC = 11,/* int32  [nblk][256]  per block, the vertex (storage) ids it stages: the vertices of its cells in (cell,
                                                 local vertex) order of first appearance, then the apex vertices of the coupled
                                                 neighbours (in-block ones included) in (cell, facet) order; 0 padded                  */
    KNP_DT_RU_VLOC = 12,  /* uint8  [nc_owned][8] positions in the block's vertex list: the cell's own vertices (0..3) and the apex
                                                 vertex of the neighbour behind facet i (4 + i; 0 where the facet couples nothing)     */
    KNP_DT_RU_HINV4 = 13  /* double [nc_owned][4] 2 / (h + h') of the cell and the neighbour behind facet i (0 where it couples nothing) */
};
int64_t knp_debug_table_size(knp_ctx* ctx, int which);
int knp_debug_table(knp_ctx* ctx, int which, void* out, int64_t nbytes);

/* ---- per-step coefficient updates ----------------------------------------------------------- */
int knp_update_kappa(knp_ctx* ctx);        /* KAPPA <- C, C_ELIM                (solver.py:303-306) */
int knp_update_dnphi(knp_ctx* ctx);        /* DNPHI <- PHI                      (feeds solver.py:583,593) */

/* ---- operator applies (matrix-free MatMult) --------------------------------------------------
 * fy = A_emi(KAPPA) fx  on scalar fields;   fy = A_knp(DNPHI) fx  on [n_sys] species-major fields. */
int knp_emi_apply(knp_ctx* ctx, int fx, int fy);
int knp_knp_apply(knp_ctx* ctx, int fx, int fy);

/* ---- right-hand sides ------------------------------------------------------------------------ */
int knp_emi_rhs(knp_ctx* ctx);             /* B_EMI <- L_emi(C, C_ELIM, PHI_M, I_CH)          solver.py:478 */
int knp_knp_rhs(knp_ctx* ctx);             /* B_KNP <- L_knp(C, C_PREV, C_ELIM, PHI, PHI_M, I_CH) solver.py:731 */

/* ---- solves (KSP.solve) ----------------------------------------------------------------------
 * EMI: PCG, cell-block-Jacobi (+ auxiliary-space AMG when uploaded); initial guess: extrapolated from PHI and the solve's history
 *      (below; the reference starts from PHI itself, ksp_initial_guess_nonzero).
 *      Without a residual target (knp_emi_residual_target(ctx, 0), the state after knp_ctx_create): PETSc's default test on the
 *      preconditioned norm, ||M^-1 r|| <= max(rtol ||M^-1 b||, atol) (solver.py:425-444); res = {||M^-1 r0||, ||M^-1 r||, ||M^-1 b||}.
 *      With a residual target r_abs > 0 (what knpemidg.Solver uses; csrc/krylov.hip: cg_converged) the solve ends when BOTH
 *        (i)  ||(b - A phi) / vol||_8 <= r_abs      -- the TRUE residual in the order-8 norm of its density (sum_K (|r_K| / vol_K)^8)^(1/8),
 *             a sum-type stand-in for the max norm; the caller derives r_abs from the accuracy wanted in the concentrations, and
 *        (ii) ||phi - phi_k||_A <= rtol ||phi||_A   -- the energy-norm error of the iterate, estimated from the CG coefficients through the
 *             Hestenes-Stiefel identity ||x - x_k||_A^2 = sum_{j >= k} alpha_j (r_j . z_j), which holds for ANY SPD preconditioner
 *             (the tail of the sum extrapolated with the decay rate of its terms smoothed over the last quarter of the iterations)
 *      hold, at the latest when ||M^-1 r|| <= 1e-11 ||M^-1 b|| (targets below what fp64 reaches must not loop forever); atol is not used;
 *      res = {||r0 / vol||_8, ||r / vol||_8, estimated ||phi - phi_k||_A / ||phi||_A}.  Neither (i) nor (ii) depends on the preconditioner.
 * KNP: per-species BiCGStab (or GMRES, knp_set_knp_krylov), same preconditioner family, TRUE residual: converged when
 *      ||r / vol||_8 <= max(20 rtol ||b / vol||_8, atol) -- order-8 norms of the residual and load DENSITIES: the concentrations are asked
 *      for in the max norm, and their max-norm error was measured at 0.03-0.055 of that ratio on uniform AND on sliver-ridden meshes
 *      (csrc/krylov.hip, profiles/r03_knp_norms_*.txt), i.e. the test asks for an estimated relative max-norm error of about rtol; the
 *      factor 20 (KNP_D8_FACTOR) applies to whatever rtol is passed (callers that mean the residual itself, e.g. a direct-solve
 *      emulation, divide it out); at least min_it iterations (ksp_min_it, solver.py:686); initial guess: extrapolated from C and the
 *      solve's history (below).
 *      res per system = {||r0 / vol||_8, ||r / vol||_8, ||b / vol||_8} (KNP_KNP_NORM2=1: the cell-volume-weighted 2-norms instead).
 * Initial guess (csrc/solve.hip: extrapolate_guess).  Each solve keeps a history h1, h2 of the fields it was STARTED from and a count
 *      nh of valid entries.  With x the content of PHI (C) when the solve is called: nh = 0: the guess is x; nh >= 1: 2 x - h1 (one
 *      rounding); with KNP_EXTRAPOLATE_ORDER=2 (or _EMI / _KNP for one solve) and nh = 2: 3 (x - h1) + h2.  Then h2 <- h1 (order 2, or
 *      KNP_FUSE_EXTRAP=0), h1 <- x, nh <- min(nh + 1, 2).  knp_upload of PHI sets nh = 0 for the EMI solve, knp_upload of C for the KNP
 *      solve; nothing else does (not knp_set_params, not the other uploads; knp_state_load restores the saved count).  So the
 *      first solve after an upload of U starts from U and makes U the history point h1: the second one starts from 2 x_1 - U, with x_1
 *      the first solution.  KNP_EXTRAPOLATE=0 starts every solve from the field itself (2: EMI only, 3: KNP only), as does the
 *      manufactured-solution mode (splitting = 2).  A solve with maxit = 0 leaves the guess in the field and returns -3.
 *      The lagged cell-block inverses (rebuilt from the current coefficients every KNP_BJ_LAG = 8 solves; a KNP solve on the
 *      drift-free class table sets their age to 0 instead, so the first solve that falls back to them rebuilds them) and the spectral bound of
 *      the Chebyshev cell-block smoother are reset by knp_set_params and by knp_upload of C, C_ELIM, PHI or KAPPA.
 * niter: iterations (EMI: 1 int, KNP: n_sys ints).  Returns -3 if not converged within maxit (ksp_error_if_not_converged, solver.py:428).
 * knp_emi_residual_target: r_abs > 0 arms the error-controlled stop above for the following EMI solves; 0 restores PETSc's test.
 *      Every rank of a partitioned run must pass the same number (knp_allreduce_sum). */
int knp_emi_residual_target(knp_ctx* ctx, double r_abs);
/* knp_knp_early_stop: factor in [0, 1); 0 (the state after knp_ctx_create) = a BiCGStab solve never stops before `min_it` iterations.  With
 * factor > 0 it also stops as soon as its residual is `factor` times UNDER the tolerance -- the floor exists to keep the per-step errors of a
 * quiet phase (the extrapolated initial guess already passes the test) far below the tolerance, which such a residual does by itself.
 * (GMRES keeps the plain floor.)  knpemidg.Solver sets 0.01 (`solver_params.knp_early_stop`). */
int knp_knp_early_stop(knp_ctx* ctx, double factor);
/* knp_knp_load_measure: out[k] = sum over this context's owned cells of (|b_K| / vol_K)^8 of the KNP right-hand side of species k (field B_KNP
 * as knp_knp_rhs left it; with KNP_KNP_NORM2=1: |b_K|^2 / vol_K) -- the size of the load the residual target above is scaled with
 * (knpemidg/solver.py: _knp_load_norm sums over the ranks and takes the root).  Replaces a host pass over the downloaded field. */
int knp_knp_load_measure(knp_ctx* ctx, double* out);
int knp_emi_solve(knp_ctx* ctx, double rtol, double atol, int maxit, int check_every, int* niter, double* res);
int knp_knp_solve(knp_ctx* ctx, double rtol, double atol, int maxit, int min_it, int check_every, int* niter, double* res);
/* Krylov method of knp_knp_solve: 0 = BiCGStab (default: 4 operator applies and no stored basis per iteration), 1 = right-preconditioned
 * restarted GMRES(restart), restart in 2..30 -- the reference's KSP type and restart length (ksp_type gmres, ksp_gmres_restart 30,
 * src/knpemidg/solver.py:684-701); same preconditioner and the same stopping test on the true residual either way.  niter of a GMRES
 * solve counts Arnoldi steps (= preconditioner applications). */
int knp_set_knp_krylov(knp_ctx* ctx, int method, int restart);
/* DG-level smoother of the EMI preconditioner (stands in for pc_type hypre on BB_emi, solver.py:433, 505): 1 = two-step Chebyshev
 * block-Jacobi (one more operator apply per PCG iteration, fewer iterations), 0 = plain cell-block-Jacobi, -1 = default (1 for DG-P1).
 * Every rank of a partitioned run must pass the same value (the preconditioner has to be one symmetric operator). */
int knp_set_emi_dg_smoother(knp_ctx* ctx, int chebyshev);

/* ---- auxiliary-space AMG preconditioner (stands in for pc_type hypre, solver.py:433, 688) ---------------
 * M^-1 = cell-block-Jacobi + P Ac^+ P^T with Ac the conforming (membrane-broken) P1 operator; the hierarchy is
 * built on the host (knpemidg/amg.py) and uploaded level by level.  which: 0 = EMI, 1 + k = KNP species k.
 *  knp_amg_begin : DG -> conforming dof map [nc*nd] and its inverse as a CSR list (conforming dof -> owned DG dofs, ascending;
 *                  cg_ptr = cg_idx = NULL: derived here)
 *  knp_amg_level : one level (A csr, inverse diagonal, spectral radius of D^-1 A, Chebyshev degree / lower
 *                  fraction; P [n x ncoarse] and R = P^T as CSR; ncoarse = 0 on the last level)
 *  knp_amg_finish: dense pseudo-inverse [n*n] of the last level; arms the preconditioner
 *  knp_amg_clear : back to plain block-Jacobi */
int knp_amg_begin(knp_ctx* ctx, int which, int64_t ncg, const int32_t* dg2cg, const int32_t* cg_ptr, const int32_t* cg_idx);
/* Optional, between knp_amg_begin and the first knp_amg_level: the hierarchy of slot `which` (>= 1) preconditions the
 * first ncol KNP species together (their level vectors become [ncol][n] and one chain of kernels carries all columns);
 * slots of the other species then stay empty.  Used when the species' diffusion coefficients are close. */
int knp_amg_columns(knp_ctx* ctx, int which, int ncol);
int knp_amg_level(knp_ctx* ctx, int which, int64_t n, const int32_t* rowptrA, const int32_t* colA, const double* valA,
                  const double* dinv, double rho, int cheb_degree, double cheb_lower, int64_t ncoarse,
                  const int32_t* rowptrP, const int32_t* colP, const double* valP,
                  const int32_t* rowptrR, const int32_t* colR, const double* valR);
int knp_amg_finish(knp_ctx* ctx, int which, int64_t n, const double* pinv);
int knp_amg_finish_f32(knp_ctx* ctx, int which, int64_t n, const float* pinv);   /* the same, inverse already in fp32 */
int knp_amg_clear(knp_ctx* ctx, int which);
/* Partitioned runs: ROW-DISTRIBUTED finest conforming level (the reference's BoomerAMG is row-distributed on every level under MPI,
 * src/knpemidg/solver.py:433, 688, with PETSc's VecScatter behind MatMult, :529, :789).  Each rank holds the conforming dofs of its own
 * cells (+ of the membrane facets assigned to it) in local numbering and the level-0 matrix SUB-ASSEMBLED from those cells / facets, so
 * that a product is a per-rank partial sum; partial sums at dofs shared by several ranks are exchanged point to point
 * (2 messages per peer) and added in rank order.  Levels >= 1 stay replicated behind ONE all-reduce of the level-1 residual per V-cycle.
 *  knp_amg_interface: the shared-dof tables (every rank of the communicator calls it, once per conforming space): peers[p] shares
 *                     counts[p] dofs; idx = their local numbers grouped by peer, ascending global dof within a peer; uvtx / aptr / asrc:
 *                     per distinct shared dof the message positions of its other owners in ascending rank order, -1 = own value.
 *  knp_amg_dist0    : between knp_amg_begin and the first knp_amg_level of a hierarchy uploaded in that local form. */
int knp_amg_interface(knp_ctx* ctx, int64_t n_local, int npeers, const int32_t* peers, const int64_t* counts, const int32_t* idx,
                      int64_t nuniq, const int32_t* uvtx, const int32_t* aptr, const int32_t* asrc);
int knp_amg_dist0(knp_ctx* ctx, int which);

/* ---- step III (solver.py:808-845) -------------------------------------------------------------
 * C_PREV <- C ; PHI_M <- facet-avg(phi_i - phi_e) ; C_ELIM <- -(sum z_k c_k + rho)/z_N ; E <- Nernst. */
int knp_step_updates(knp_ctx* ctx);
int knp_nernst(knp_ctx* ctx);              /* E only, from the current C / C_ELIM (solver.py:299-300) */
/* Picard variant (solve_for_time_step_picard, solver.py:850-927): per Picard level C_ELIM and E from the current C;
 * knp_max_abs_diff = inf-norm of the difference of two nodal fields (the eps of solver.py:879-880). */
int knp_picard_updates(knp_ctx* ctx);
int knp_max_abs_diff(knp_ctx* ctx, int field_a, int field_b, double* out);
/* FACET_TMP[slot] <- facet average of the plus (side 0, ECS-like) or minus (side 1) trace of a nodal field;
 * species indexes into [n_sys] fields (update_ode hook, examples/idealized-geometries/run_3D.py:39-51).  Several slots, so
 * that consecutive projections (K_e, Na_i, ...) do not overwrite each other before they are consumed. */
#define KNP_FACET_TMP_SLOTS 4
int knp_facet_trace(knp_ctx* ctx, int field, int species, int side, int slot);

/* ---- time-series recorder ------------------------------------------------------------------------
 * Samples probe, membrane and region quantities on the device, so that a run without field output still yields the traces the
 * reference's figure scripts compute from results.h5 (examples/idealized-geometries/make_figures_3D.py:28-168: point values of phi
 * and every concentration, the area-averaged phi_M / E_K / E_Na over a few membrane facets, subdomain integrals).  One sample is one
 * row of knp_rec_channels doubles plus its time in a device buffer of `capacity` rows; the row counter lives on the device.
 * Row layout:
 *   per probe   : phi, the n_sys solved concentrations, the eliminated one       = sum_a w[a] u[cell*nd + a]
 *   per set     : weighted mean of PHI_M, of E[k] and of I_CH[k], k < n_ions      (1 + 2 n_ions values)
 *   per region  : integral of c_k dx, k < n_ions (eliminated ion last), then the volume mean of phi; exact nodal weights
 *                 (P1: vol/(d+1); P2 triangle: 0 on vertices, 1/3 on edge nodes; P2 tetrahedron: -1/20 and 1/5)
 *   per set     : weighted means of ODE state columns, one per requested state name -- only after knp_rec_add_states, and behind
 *                 the region block, so that every offset above is what it is without them
 * Sums run in a fixed order and without floating-point atomics: the same inputs give the same bits.
 *  knp_rec_create  : point_cell[n_points] containing cell and point_w[n_points][nd] basis values at the point (P2: local dof order
 *                    of knp_set_tabulation); set s = facets set_facet[set_ptr[s] .. set_ptr[s+1]) with weights set_w (summing to 1
 *                    per set; facet ids are the caller's); region[nc] in [0, n_regions) or 255 = not counted, n_regions <= 16,
 *                    vol[nc] cell volumes (ghost cells are never counted).  Cell-indexed arguments are in DEVICE cell order.  One
 *                    recorder per context: a second call replaces the first.  A cell outside [0, nc_owned), a facet that is not a
 *                    membrane facet, an empty set or a region id >= n_regions other than 255 fails with a message and launches nothing.
 *  knp_rec_sample  : appends one row for time t; asynchronous, on the context's stream; -5 when `capacity` rows wait to be read
 *  knp_rec_read    : synchronises, copies the waiting rows (rows_out[capacity][channels], t_out[capacity]; *n_rows of them are
 *                    valid) in one device-to-host transfer and empties the buffer
 *  knp_rec_channels: doubles per row (< 0 without a recorder; state channels included once knp_rec_add_states has run)
 *
 * Optional, after knp_rec_create (which alone leaves rows, offsets and launches exactly as described above):
 *  knp_rec_add_states: appends n_channels channels BEHIND the region block, channel s = sum over its entries
 *                    i in [chan_ptr[s], chan_ptr[s+1]) of entry_w[i] * states(entry_handle[i])[entry_row[i]][entry_col[i]] -- weighted
 *                    means of ODE state columns such as the gating variables n, m, h over a membrane set that may span several
 *                    handles.  Summed in list order by one workgroup per channel (k_rec_states), one launch per sample.  Every entry
 *                    is checked before anything is uploaded: handle exists, 0 <= row < n, 0 <= col < ns, and the weights of a channel
 *                    sum to 1 within 1e-12; a failure leaves the recorder as it was.  Not while samples wait to be read.
 *                    Timing: the solver steps the membrane ODEs of step k before the PDE solves of step k, so the row sampled at the
 *                    end of step k holds the states AFTER ODE step k, the pairing the reference's saved fields have.
 *  knp_rec_add_map : per-facet activation map of the n given membrane facets (caller's ids), persistent on the device: prev, t_act,
 *                    t_repol, peak, t_peak (doubles) and n_up (int32).  Per sample (k_rec_map, one thread per facet, one launch), with
 *                    v0 = prev at the previous sample's time t0 and v1 = PHI_M[f] at this sample's time t1:
 *                      v0 < thr && v1 >= thr                                   : ++n_up; t_act = t0 + (thr - v0) / (v1 - v0) (t1 - t0) if unset
 *                      t_act set, t_repol unset, v0 >= thr_r && v1 < thr_r     : t_repol by the same interpolation with thr_r
 *                      v1 > peak                                               : peak = v1, t_peak = t1
 *                      prev = v1
 *                    t0 lives on the device next to the row counter; a refused sample (buffer full) changes nothing.  A facet that is
 *                    not a membrane facet, n < 1 or a non-finite threshold fails before anything is uploaded.
 *  knp_rec_map_arm : t_act = t_repol = NaN, n_up = 0, peak = prev = PHI_M now, t_peak = t0; asynchronous.  knp_rec_sample refuses to
 *                    sample an unarmed map.
 *  knp_rec_map_read: synchronises and copies t_act, t_repol, peak, t_peak, n_up ([n] each) in one device-to-host transfer; never
 *                    part of knp_rec_read
 *
 * Partition mode, for the ranks of a partitioned run (one context per rank; knpemidg/recorder.py: localize_tables).  Every rank holds
 * the tables of what it OWNS -- a probe: the rank that owns its cell; a membrane facet: the rank that owns its first cell; a cell's
 * volume: its owner -- with the weights of the GLOBAL sets, and writes its PARTIAL row with the same kernels and launches; nothing
 * is communicated per sample.  The row layout above is unchanged.  The three calls below replace their namesakes (mixing the two
 * families on one recorder fails); every other call is shared.  Without a communicator they work on the rank's part alone.
 *  knp_rec_create_part    : as knp_rec_create, except: point_cell may be -1 (a probe another rank owns: its channels are an exact
 *                    0.0 here); a set may be empty (0.0); inv_rvol[n_regions] = 1 / GLOBAL region volume (finite, >= 0) replaces
 *                    the volume summed over this rank's cells.  Everything else -- cells in [0, nc_owned), membrane facets, region
 *                    ids -- is validated as there, before anything is uploaded.
 *  knp_rec_add_states_part: as knp_rec_add_states, except: a channel may be empty and its weights (each >= 0) sum to <= 1.
 *  knp_rec_add_map_part   : n >= 0 membrane facets of this rank (caller's ids); facet i is entry positions[i] of the n_global >= 1
 *                    entries of the global map (distinct, in [0, n_global)).  The per-sample kernels run on the rank's n facets.
 *  knp_rec_read    : with a communicator, first sums the waiting rows over the ranks in place on the device -- one all-reduce of
 *                    rows x channels doubles on the context's stream and main communicator (shm transport: in pieces of the
 *                    reduction slot, summed in rank order, the same bits on every rank); the times are not reduced.  COLLECTIVE:
 *                    every rank calls it after the same number of samples, with the same capacity.
 *  knp_rec_map_read: n = n_global.  k_rec_map_spread (one thread per global entry) writes the rank's five arrays, n_up as a double,
 *                    to their global positions in a staging buffer and 0.0 elsewhere, so that an owner's NaN survives; one
 *                    all-reduce of 5 n_global doubles, one copy.  COLLECTIVE.  Every rank receives the whole map. */
int knp_rec_create(knp_ctx* ctx, int64_t capacity, int64_t n_points, const int32_t* point_cell, const double* point_w,
                   int64_t n_sets, const int64_t* set_ptr, const int32_t* set_facet, const double* set_w,
                   int n_regions, const uint8_t* region, const double* vol);
int knp_rec_sample(knp_ctx* ctx, double t);
int knp_rec_read(knp_ctx* ctx, int64_t* n_rows, double* t_out, double* rows_out);
int64_t knp_rec_channels(knp_ctx* ctx);
int knp_rec_add_states(knp_ctx* ctx, int64_t n_channels, const int64_t* chan_ptr, const int32_t* entry_handle, const int64_t* entry_row,
                       const int32_t* entry_col, const double* entry_w);
int knp_rec_add_map(knp_ctx* ctx, int64_t n, const int32_t* facets, double threshold, double repolarisation);
int knp_rec_map_arm(knp_ctx* ctx, double t0);
int knp_rec_map_read(knp_ctx* ctx, int64_t n, double* t_act, double* t_repol, double* peak, double* t_peak, int32_t* n_up);
int knp_rec_destroy(knp_ctx* ctx);
int knp_rec_create_part(knp_ctx* ctx, int64_t capacity, int64_t n_points, const int32_t* point_cell, const double* point_w,
                        int64_t n_sets, const int64_t* set_ptr, const int32_t* set_facet, const double* set_w,
                        int n_regions, const uint8_t* region, const double* vol, const double* inv_rvol);
int knp_rec_add_states_part(knp_ctx* ctx, int64_t n_channels, const int64_t* chan_ptr, const int32_t* entry_handle,
                            const int64_t* entry_row, const int32_t* entry_col, const double* entry_w);
int knp_rec_add_map_part(knp_ctx* ctx, int64_t n_global, int64_t n, const int32_t* facets, const int64_t* positions, double threshold,
                         double repolarisation);

/* ---- fields on a regular voxel grid (csrc/grid.hip) ---------------------------------------
 * Between the recorder's few probes and a download of every DoF: phi and the concentrations sampled at the points of a regular
 * grid, a dense frame [n_fields][nz][ny][nx] ([n_fields][ny][nx] in 2D; x runs fastest) whose size the caller chooses.  Point i of
 * axis k is lo[k] + i h[k]; an axis with shape[k] = 1 sits at lo[k] (a slice of a 3D mesh).  The owner of a point is, among the cells
 * whose smallest barycentric coordinate is >= -tol (and, with n_tags > 0, whose subdomain tag is one of tags), the one with the lowest
 * id in the CALLER's numbering (knp_state_cell_order; the rule of knpemidg/recorder.py: locate_points); a point no cell contains has
 * owner -1, tag -1 and NaN in every field -- not an error, a grid may stick out of the mesh.  Value = sum_a w_a(lambda) u[cell nd + a]
 * with the nodal basis in the local dof order of knp_set_tabulation.  The grid holds no step-to-step state: knp_state_describe
 * reports the same blocks with and without one.
 *  knp_grid_create : field ids: 0 = phi, 1 + k = solved concentration k, n_ions = the eliminated ion; f32 != 0: frames in fp32.
 *                    Everything is checked before anything is allocated (finite lo and h, h > 0 where shape > 1, shape >= 1, fewer
 *                    than 2^31 points, tol >= 0, at most 8 tags, known field ids, at most 8 grids per context); a failure leaves the
 *                    context as it was.  Runs the locate pass (one thread per cell, integer atomicMin per point: deterministic) and the
 *                    weights pass, and waits for them.  Returns the handle >= 0, or a negative status; -7 with a communicator active
 *                    (several ranks), without entering a collective.
 *  knp_grid_create_derived : knp_grid_create plus n_derived quantities evaluated in the owner cell, with that cell's D (DG gradients are
 *                    one-sided: on a facet, an edge, a vertex or the membrane the owner decides the side, as it decides the value;
 *                    tags therefore give ECS-only or ICS-only fluxes).  kind[q]: KNP_GD_EFIELD  -grad phi;  KNP_GD_FLUX_DIFFUSIVE
 *                    -D_k grad c_k;  KNP_GD_FLUX  J_k = -D_k grad c_k - z_k D_k psi c_k(p) grad phi, psi = F / (R T);  KNP_GD_CURRENT
 *                    F sum_k z_k J_k over every ion.  ion[q] = 0 .. n_ions - 1 (n_ions - 1: the eliminated ion, C_ELIM); ignored for
 *                    EFIELD and CURRENT.  Units are those of knp_set_params.  A frame is [n_fields nodal planes][per derived quantity:
 *                    d component planes, x first][npts]; NaN in every component without an owner.  n_fields may be 0 here.  Also
 *                    refused before anything is allocated: an unknown kind, an ion outside 0 .. n_ions - 1, nothing selected, more
 *                    than 2 n_ions + 2 derived quantities, a context whose parameters were never set (knp_set_params).
 *                    knp_grid_create is this call with n_derived = 0.  A grid with derived quantities runs the nodal kernel for its
 *                    nodal planes and then one more kernel; knp_grid_timing's sample_ms spans both.
 *  knp_grid_points : owner[npts] (caller's cell ids) and tag[npts] of the points; either may be null
 *  knp_grid_sample : one frame of the fields as they are now: kernel, asynchronous copy into one of two pinned host buffers and an
 *                    event, all on the context's stream; -5 while two frames wait to be fetched
 *  knp_grid_fetch  : waits for the event of the oldest waiting frame only and copies it to out[bytes], bytes = (n_fields + d n_derived) x npts x 8 (4)
 *  knp_grid_timing : device milliseconds of the locate and weights passes, and of the kernel and the copy of the last fetched frame */
int knp_grid_create(knp_ctx* ctx, const double* lo, const double* h, const int64_t* shape, double tol, int n_tags, const uint32_t* tags,
                    int n_fields, const int32_t* fields, int f32);
typedef enum { KNP_GD_EFIELD = 0, KNP_GD_FLUX = 1, KNP_GD_FLUX_DIFFUSIVE = 2, KNP_GD_CURRENT = 3 } knp_grid_derived;
int knp_grid_create_derived(knp_ctx* ctx, const double* lo, const double* h, const int64_t* shape, double tol, int n_tags,
                            const uint32_t* tags, int n_fields, const int32_t* fields, int n_derived, const int32_t* kind,
                            const int32_t* ion, int f32);
int knp_grid_points(knp_ctx* ctx, int grid, int32_t* owner, int32_t* tag);
int knp_grid_sample(knp_ctx* ctx, int grid);
int knp_grid_fetch(knp_ctx* ctx, int grid, void* out, size_t bytes);
int knp_grid_destroy(knp_ctx* ctx, int grid);
int knp_grid_timing(knp_ctx* ctx, int grid, float* locate_ms, float* weights_ms, float* sample_ms, float* copy_ms);

/* ---- membrane-surface snapshots (csrc/surface.hip) ----------------------------------------
 * Per selected membrane facet (the caller's facet ids, ascending) a frame [n_fields + n_states][n] of facet quantities, one
 * thread per facet.  kind[q] / ion[q] of field plane q:
 *   KNP_SF_PHI_M       PHI_M[f]                       KNP_SF_I_CH_TOTAL  sum_k I_CH[k nf + f], added in ion order
 *   KNP_SF_E           E[ion nf + f]                  KNP_SF_TRACE_E     facet mean of the trace from cell_e (the `plus` side) ...
 *   KNP_SF_I_CH        I_CH[ion nf + f]               KNP_SF_TRACE_I     ... and from cell_i (`minus`) of phi (ion -1) or of concentration `ion`
 * (ion n_ions - 1 is the eliminated one; the facet mean is what knp_facet_trace writes: P1 the mean of the facet's vertex values, P2
 * the exact mean of the quadratic).  State plane s holds, per facet, column state_col of row state_row of the state table of ODE handle
 * state_handle -- tables [n_states][n]; handle -1: the facet's model has no such state, the plane holds NaN there.
 *  knp_surf_create : returns a handle (0 .. 3) or a negative code.  Everything is checked on the host before anything is allocated or
 *                    uploaded and a failure leaves the context as it was: -7 with several ranks; -1 for facets that are not ascending
 *                    or not membrane facets of the context, unknown kinds, ions out of range, unknown ODE handles, rows or columns
 *                    outside their table, parameters never set (E, I_ch), a fifth sampler.  f32 != 0: frames in fp32 (the fp64 value
 *                    rounded once).
 *  knp_surf_sample : one frame of the state as it is now: kernel, asynchronous copy into one of two pinned host buffers and an event;
 *                    -5 when both buffers wait to be fetched
 *  knp_surf_fetch  : waits for the event of the oldest waiting frame only and copies it to out[bytes], bytes = planes x n x 8 (4)
 *  knp_surf_timing : device milliseconds of the kernel and the copy of the last fetched frame
 * A sampler holds no step-to-step state: knp_state_describe is the same with and without one. */
typedef enum { KNP_SF_PHI_M = 0, KNP_SF_E = 1, KNP_SF_I_CH = 2, KNP_SF_I_CH_TOTAL = 3, KNP_SF_TRACE_E = 4, KNP_SF_TRACE_I = 5 } knp_surf_kind;
int knp_surf_create(knp_ctx* ctx, int64_t n, const int32_t* facets, int n_fields, const int32_t* kind, const int32_t* ion, int n_states,
                    const int32_t* state_handle, const int64_t* state_row, const int32_t* state_col, int f32);
int knp_surf_sample(knp_ctx* ctx, int surf);
int knp_surf_fetch(knp_ctx* ctx, int surf, void* out, size_t bytes);
int knp_surf_destroy(knp_ctx* ctx, int surf);
int knp_surf_timing(knp_ctx* ctx, int surf, float* sample_ms, float* copy_ms);

/* ---- volume-field snapshots on the mesh (csrc/fieldmesh.hip) ---------------------------------
 * Per output node the arithmetic mean of a list of nodal values; a frame is [n_fields][n_nodes].  The lists arrive as CSR: ptr
 * [n_nodes + 1] and entries [ptr[n_nodes]][2] = (cell in the context's own -- device -- cell order, local dof in the order of
 * knp_set_tabulation); the library forms the addresses with its own cell stride.  The value of a node is the first listed value, the
 * further ones added one by one in list order, then one division by the list's length, all in fp64 (a list of length one gives the
 * nodal value's bits).  kind[q] / ion[q] of plane q: KNP_FM_PHI (ion ignored) or KNP_FM_C with ion 0 .. n_ions - 1 (the last is the
 * eliminated one).
 *  knp_fieldmesh_create : writes the handle (0 .. 3) and returns 0, or a negative code.  Everything is checked on the host before
 *                         anything is allocated or uploaded and a failure leaves the context as it was: -7 with several ranks; -1
 *                         for a ptr that does not start at 0, is not strictly increasing (an empty list), a cell outside the owned
 *                         cells, a dof outside 0 .. nd - 1, an unknown kind, an ion out of range, no plane or more than
 *                         KNP_MAX_IONS + 1, a fifth sampler.  f32 != 0: frames in fp32 (the fp64 value rounded once).
 *  knp_fieldmesh_sample : one frame of the state as it is now: kernel, asynchronous copy into one of two pinned host buffers and an
 *                         event; -5 when both buffers wait to be fetched
 *  knp_fieldmesh_fetch  : waits for the event of the oldest waiting frame only and copies it to out[bytes], bytes = n_fields x
 *                         n_nodes x 8 (4)
 *  knp_fieldmesh_timing : device milliseconds of the kernel and the copy of the last fetched frame
 * A sampler holds no step-to-step state: knp_state_describe is the same with and without one. */
typedef enum { KNP_FM_PHI = 0, KNP_FM_C = 1 } knp_fieldmesh_kind;
int knp_fieldmesh_create(knp_ctx* ctx, int64_t n_nodes, const int64_t* ptr, const int32_t* entries, int n_fields, const int32_t* kind,
                         const int32_t* ion, int f32, int* handle);
int knp_fieldmesh_sample(knp_ctx* ctx, int fieldmesh);
int knp_fieldmesh_fetch(knp_ctx* ctx, int fieldmesh, void* out, size_t bytes);
int knp_fieldmesh_destroy(knp_ctx* ctx, int fieldmesh);
int knp_fieldmesh_timing(knp_ctx* ctx, int fieldmesh, float* sample_ms, float* copy_ms);

/* ---- checkpoint of the step-to-step state (csrc/state.hip; DESIGN.md section 4.3 lists every member saved or rebuilt).
 * A snapshot is one host buffer: a 32-byte prologue (magic "KNPSTATE", version, block count, payload bytes), the block table
 * (one knp_state_block per block) and the payloads at the table's offsets.  A block is [ncomp][count][width] elements:
 *   KNP_SK_CELL_DOF        count = cells, width = values per cell; in the CALLER's cell numbering (knp_state_cell_order)
 *   KNP_SK_FACET           count = facets (the caller's numbering is the device's)
 *   KNP_SK_MEMBRANE_FACET  count = nodes of one membrane model or facets of the recorder's map, in the order they were created with
 *   KNP_SK_OPAQUE          counters and small device buffers, no mesh meaning
 * Device blocks are packed by one gather kernel per family into one staging buffer that crosses the bus in one copy through pinned
 * memory; knp_state_load runs the scatter kernels the other way.  Neither goes through knp_upload, so the history counters of the
 * extrapolated initial guesses, the ages of the lagged block inverses and their spectral bounds come back as saved; KAPPA is
 * recomputed from the restored concentrations and the state-independent KNP block table is rebuilt before the inverses land.
 *  knp_state_cell_order: order[d] = caller's id of device cell d (a permutation of 0..nc-1; null = identity, the default)
 *  knp_state_describe  : writes up to cap table entries, returns the number of blocks (< 0: error); *bytes = size of a snapshot
 *  knp_state_save      : bytes must be the size knp_state_describe reports
 *  knp_state_load      : -8 when the buffer's block table differs from this context's (cell count, degree, ion count, membrane-model
 *                        layout, recorder configuration): nothing has been touched then.  Call it after the last knp_set_params.
 *  Both return -7 with a communicator active: snapshots of several ranks are not supported.
 *  knp_state_timing    : device milliseconds of the pack kernels and of the bus copy of the last save or load */
enum knp_state_kind { KNP_SK_OPAQUE = 0, KNP_SK_CELL_DOF = 1, KNP_SK_FACET = 2, KNP_SK_MEMBRANE_FACET = 3 };
enum knp_state_type { KNP_ST_F64 = 0, KNP_ST_F32 = 1, KNP_ST_I32 = 2, KNP_ST_I64 = 3 };
typedef struct knp_state_block {
    int32_t id, kind, type, ncomp;
    int64_t count, width;
    int64_t offset;              /* bytes from the start of the snapshot */
} knp_state_block;
#define KNP_STATE_PROLOGUE 32
int knp_state_cell_order(knp_ctx* ctx, const int64_t* order);
int64_t knp_state_describe(knp_ctx* ctx, knp_state_block* out, int64_t cap, int64_t* bytes);
int knp_state_save(knp_ctx* ctx, void* host_buf, size_t bytes);
int knp_state_load(knp_ctx* ctx, const void* host_buf, size_t bytes);
int knp_state_timing(knp_ctx* ctx, float* pack_ms, float* copy_ms);

/* ---- membrane ODEs: batched device integrator replacing the per-facet LSODA loop of
 * MembraneModel.step_lsoda (membrane.py:84-119).  model: 1 = Hodgkin-Huxley + stimulus (examples/idealized-geometries/mm_hh.py),
 * 2 = without (mm_hh_no_stim.py), 3 = EMIx neuron (examples/emix-simulations/mm_hh.py), 4 = EMIx glia (mm_glial.py), 5 = passive
 * leak (examples/rat-neuron/mm_leak.py), 6 = the ODE-only EMIx calibration system (examples/emix-simulations/mm_calibration.py).  Tables are [n][ns] states and [n][np] parameters in the reference's column layout.
 *  knp_ode_create  : returns a handle >= 0; facets[n] = facet id of every ODE node
 *  knp_ode_table   : what 0 = states, 1 = parameters; upload != 0 copies host -> device, else device -> host
 *  knp_ode_exchange: table column <- facet field (to_facet = 0, set_state/set_parameter) or facet field <- table
 *                    column (to_facet = 1, get_state/get_parameter); offset selects the row of [n_ions][nf] fields
 *  knp_ode_exchange_multi: n such copies in ONE launch (what[k], col[k], field[k], offset[k]); a membrane step moves V, E_k,
 *                    K_e, Na_i in and V, I_ch_k out (solver.py:1086-1112)
 *  knp_ode_set_stimulus: parameter columns cols[k] take values[k] on the rows with mask[row] != 0 at the start of EVERY
 *                    knp_ode_step (the reference re-imposes the stimulus every step, membrane.py:98-104); 0 entries clears
 *  knp_ode_step    : adaptive Dormand-Prince 5(4) from t0 to t0+dt per node (rtol 1e-8, atol 0: membrane.py:112).
 *                    Asynchronous: a node that fails (`assert success`, membrane.py:113) raises a device flag that the next
 *                    knp_emi_solve / knp_knp_solve status poll, knp_ode_table or knp_sync reports as -4 */
int knp_ode_create(knp_ctx* ctx, int model, int64_t n, const int32_t* facets, int ns, int np, const double* states,
                   const double* params);
int knp_ode_table(knp_ctx* ctx, int handle, int what, int upload, double* host);
int knp_ode_exchange(knp_ctx* ctx, int handle, int what, int col, int field, int64_t offset, int to_facet);
int knp_ode_exchange_multi(knp_ctx* ctx, int handle, int n, const int32_t* what, const int32_t* col, const int32_t* field,
                           const int64_t* offset, int to_facet);
int knp_ode_set_stimulus(knp_ctx* ctx, int handle, int n_entries, const int32_t* cols, const double* values, const uint8_t* mask);
int knp_ode_step(knp_ctx* ctx, int handle, double t0, double dt, double rtol, double atol);
/* Runtime-compiled right-hand sides (a model module's HIP_RHS, knpemidg/ode_rtc.py builds the translation unit around
 * csrc/ode_dp5.hpp, the integrator of knp_ode_step):
 *  knp_ode_rtc_compile: hipRTC for gfx950 with the library's code generation settings; host only (no context, no device).
 *                       *code / *size: the code object (release with knp_ode_rtc_free); log[logcap]: diagnostics and the
 *                       resource-usage remarks (VGPRs, scratch).  Non-zero on failure, with the compiler's log.
 *  knp_ode_register   : loads such a code object on the context's device; returns a model id >= 1000 for knp_ode_create
 *                       (which checks ns / np against it) and knp_ode_step (same launch shape, arguments, stream and failure
 *                       flag as the built-in models); the modules are unloaded with the context */
int knp_ode_rtc_compile(const char* src, const char* name, void** code, size_t* size, char* log, size_t logcap);
void knp_ode_rtc_free(void* code);
int knp_ode_register(knp_ctx* ctx, const void* code, size_t size, const char* kernel_name, int ns, int np);
/* A second integrator beside Dormand-Prince for stiff models (csrc/ode_stiff.hpp): the extrapolated linearly implicit Euler method,
 * order 8, with a forward-difference Jacobian; at most 11 states.  Same tables, stimulus, step-size carry-over, stream, asynchrony and
 * failure flag as the default.
 *  knp_ode_set_method    : method 0 = Dormand-Prince 5(4) (the default of knp_ode_create), 1 = stiff; knp_ode_step dispatches on it.
 *                          -1 and the set unchanged for any other value, for more than 11 states under method 1, and for a
 *                          registered model without a kernel of that method
 *  knp_ode_register_method: loads the code object of a model's kernel for `method` (knpemidg/ode_rtc.py: source(ode, method)).
 *                          model >= 1000: attaches it to that registered model (same ns / np, no kernel of that method yet) and
 *                          returns its id; model < 0: registers a new model that has this kernel only.  knp_ode_register is
 *                          method 0 on a new model
 *  knp_ode_stats         : out[4] = accepted steps, rejected steps, right-hand-side calls (Jacobian columns included) and Jacobians,
 *                          summed over the nodes and the knp_ode_step calls since knp_ode_create; only the stiff kernel counts.
 *                          Waits for the stream (and reports a pending ODE failure as -4) */
int knp_ode_set_method(knp_ctx* ctx, int handle, int method);
int knp_ode_register_method(knp_ctx* ctx, int model, int method, const void* code, size_t size, const char* kernel_name, int ns, int np);
int knp_ode_stats(knp_ctx* ctx, int handle, int64_t out[4]);

/* ---- host-side setup kernels (no device work): threaded sparse products of the preconditioner setup (knpemidg/amg.py), the
 * counterpart of the BoomerAMG setup PETSc runs inside KSPSetUp (solver.py:433, 505, 688, 767).  CSR, int32 indices, fp64 values.
 *  knp_host_spgemm: C = A B, A [n x k], B [k x m]; Cp[n+1] supplied by the caller, *Cj / *Cx allocated here (knp_host_free);
 *                   sorted columns; nthreads <= 0 = all hardware threads; -3 if C exceeds 2^31 - 1 entries
 *  knp_host_spmv  : y = A x */
int knp_host_spgemm(int64_t n, int64_t m, const int32_t* Ap, const int32_t* Aj, const double* Ax, const int32_t* Bp, const int32_t* Bj,
                    const double* Bx, int32_t* Cp, int32_t** Cj, double** Cx, int nthreads);
int knp_host_spmv(int64_t n, const int32_t* Ap, const int32_t* Aj, const double* Ax, const double* x, double* y, int nthreads);
void knp_host_free(void* p);
/* Setup kernels of the conforming auxiliary operators (knpemidg/amg.py; the reference assembles BB_emi / AA_knp with dolfin.assemble at
 * every solve, src/knpemidg/solver.py:477-479, 730-731, and hands them to BoomerAMG):
 *  knp_host_cell_gram   : vol[nc], G[nc][(dim+1)^2] = grad lambda_a . grad lambda_b of every simplex cell from vertex coordinates
 *  knp_host_segment_sum : out[p] = sum_{k in [starts[p], starts[p+1])} src[order[k]] -- per-cell blocks summed into the values of a CSR
 *                         matrix whose pattern (sort order of the entry keys) is cached */
int knp_host_cell_gram(int64_t nc, int dim, const double* coords, const int32_t* cells, double* vol, double* G, int nthreads);
int knp_host_segment_sum(int64_t nseg, const int64_t* starts, const int64_t* order, const double* src, double* out, int nthreads);
/*  knp_host_block_pattern: the cached pattern itself -- entry (c, a, b) of blocks [nc][nd][nd] lands in (dof[c][a], dof[c][b]) of an
 *                         n x n matrix; order[nc nd nd], starts[<= nc nd nd + 1], cols[<= nc nd nd], indptr[n + 1] as a stable sort of the
 *                         entry keys would give them; *nseg = number of distinct (row, column) pairs */
/* Mesh tables on the host (knpemidg/mesh.py, knpemidg/_abi.py; the reference gets them from DOLFIN's mesh topology, solver.py:85-121):
 *  knp_host_build_facets     : facet numbering by first appearance in (cell, local facet) order + the facet -> cells / local index tables
 *  knp_host_geometry_classes : classes of cells with the same shape and neighbour configuration (structured meshes) */
int64_t knp_host_build_facets(int64_t nc, int nv, const int32_t* cells, int32_t* cell_facets, int32_t* facets, int32_t* facet_cells,
                              int8_t* facet_local);
int64_t knp_host_geometry_classes(int64_t nc, const double* coords, const int32_t* cells, const int32_t* nbr, const int8_t* nbj, double quantum,
                                  int64_t max_classes, int32_t* cls, int64_t* first, int nthreads);
int knp_host_block_pattern(int64_t nc, int nd, int64_t n, const int32_t* dof, int64_t* order, int64_t* starts, int32_t* cols, int32_t* indptr,
                           int64_t* nseg, int nthreads);
/*  knp_host_sym_to_f32: the dense coarsest-level inverse after LAPACK potri -- `a` [n x n] row-major with valid numbers in its upper triangle
 *  -> the full symmetric matrix rounded to fp32 (what knp_amg_finish_f32 uploads) and its largest magnitude (NaN if an entry is not finite) */
int knp_host_sym_to_f32(int64_t n, const double* a, float* out, double* maxabs, int nthreads);
/*  knp_host_mis2_aggregate: aggregates from a distance-2 maximal independent set of a strength graph (CSR pattern, symmetric, no diagonal),
 *  Luby rounds on the priorities key[n]; agg[n] receives the aggregate of every node, the return value is their number (< 0: bad arguments) */
int64_t knp_host_mis2_aggregate(int64_t n, const int32_t* indptr, const int32_t* indices, const double* key, int64_t* agg, int nthreads);
/*  knp_host_morton_order: stable argsort of points (or, with conn, of the midpoints of the rows of conn) along a Morton curve in units of
 *  `scale` per axis -- the device numbering of cells and vertices; knp_host_cell_extent_median: that scale, the median cell extent per axis */
int knp_host_morton_order(int64_t n, int d, const double* pts, const int32_t* conn, int nv, const double* scale, int64_t* order, int nthreads);
int knp_host_cell_extent_median(int64_t nc, int nv, int d, const double* coords, const int32_t* cells, double* out);
/*  knp_host_cell_neighbours: nb[nc][nv] = cell behind local facet i (-1: none), nj[nc][nv] = that cell's local index of the facet */
int knp_host_cell_neighbours(int64_t nc, int nv, const int32_t* cell_facets, const int32_t* facet_cells, const int8_t* facet_local, int32_t* nb,
                             int8_t* nj, int nthreads);
/*  knp_host_box_marks: out[i] = 1 where the midpoint of row i of conn lies in the box [a, b] (mode 0) / on its surface within eps (mode 1) */
int knp_host_box_marks(int64_t n, int d, const double* coords, const int32_t* conn, int nv, const double* a, const double* b, double eps, int mode,
                       uint8_t* out, int nthreads);
/*  Smoothed-aggregation passes (knpemidg/amg.py: build_hierarchy), row-parallel, the numbers of the numpy / scipy lines they replace:
 *  knp_host_strength            : pattern of the strong off-diagonal couplings |a_ij| >= theta sqrt(|a_ii a_jj|)           (*Sj: knp_host_free)
 *  knp_host_smooth_prolongator  : C = P - diag(v) A P, one damped-Jacobi step on a prolongator, exact zeros dropped         (*Cj, *Cx)
 *  knp_host_truncate_prolongator: rows cut below trunc * (row maximum) and rescaled to interpolate Bc to the same values    (*Tj, *Tx) */
int knp_host_strength(int64_t n, const int32_t* Ap, const int32_t* Aj, const double* Ax, const double* diag, double theta, int32_t* Sp, int32_t** Sj,
                      int nthreads);
int knp_host_smooth_prolongator(int64_t n, int64_t m, const int32_t* Ap, const int32_t* Aj, const double* Ax, const double* v, const int32_t* Pp,
                                const int32_t* Pj, const double* Px, int32_t* Cp, int32_t** Cj, double** Cx, int nthreads);
int knp_host_truncate_prolongator(int64_t n, const int32_t* Pp, const int32_t* Pj, const double* Px, double trunc, const double* Bc, int32_t* Tp,
                                  int32_t** Tj, double** Tx, int nthreads);

/* ---- timing / sync ------------------------------------------------------------------------------ */
int knp_sync(knp_ctx* ctx);
/* Number of blocking waits of the host on the device the library has made through this context since it was created (stream and
 * event synchronisations, blocking copies): a measure of the host round trips of a time step that does not depend on timing */
long long knp_host_round_trips(knp_ctx* ctx);
int knp_timer_begin(knp_ctx* ctx);         /* records a HIP event on the context's stream */
int knp_timer_end(knp_ctx* ctx, float* ms);/* records, synchronises, returns elapsed ms */
/* Launches `reps` back-to-back applies (which: 0 = EMI, 1 = KNP) on X -> Y and returns the average
 * kernel duration measured with HIP events on the stream the kernel runs on.  Three input / output vector pairs are used in
 * rotation so that the launches are not served from the Infinity Cache. */
int knp_bench_apply(knp_ctx* ctx, int which, int reps, float* avg_ms);
/* In-solver timing of the same kernels: while enabled, every operator apply launched by the solves is bracketed by a HIP event
 * pair on the context's stream; knp_apply_timing_read synchronises, returns the average duration and the number of launches
 * since the last read (which: 0 = EMI, 1 = KNP) and resets the tally. */
int knp_apply_timing(knp_ctx* ctx, int enable);
int knp_apply_timing_read(knp_ctx* ctx, int which, float* avg_ms, int* count);

/* Which kernel knp_emi_apply (which = 0) / knp_knp_apply (which = 1) currently dispatches to, so that a measurement can name it:
 * 0 coordinate path (any mesh), 1 geometry classes + LDS staging (structured 3D P1), 2 halo-staged persistent kernel, 6 the same
 * with D read through the material table (knp_set_params found <= 16 distinct coefficient tuples), 3 (EMI) / 7 (KNP) ring-staged
 * kernels (loader wave + LDS-DMA ring + consumer waves, csrc/apply_ring.hip; the default on structured 3D P1 meshes), 8 matrix-free P2,
 * 9 assembled P2 blocks (KNP_P2_ASSEMBLED=1).  Negative on bad arguments.  No reference counterpart (measurement only). */
int knp_apply_variant(knp_ctx* ctx, int which);

/* FP64 MFMA probe of the DG-P2 path's dense facet-quadrature contraction (csrc/p2_probe.hip): variant 0 = per-thread FMA chain
 * (what the product kernels use), 1 = v_mfma_f64_16x16x4_f64 tiles.  in[ncol][26] = {jump(u)[6], kappa[6], kappa'[6], dn u[3],
 * dn u'[3], area, penalty}, out[ncol][9] = {r[6], T[3]}; returns the average kernel time over `reps` launches.  Diagnostic
 * (no counterpart in the reference): it documents why the product path keeps the vector pipe. */
int knp_probe_facet_contraction(knp_ctx* ctx, int variant, int64_t ncol, int reps, const double* in, double* out, float* avg_ms);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ------------------------------------------------
 * Replaces DOLFIN ghosting + PETSc VecGhost/MatMult scatters + KSP reductions (solver.py:16,529,789). */
int knp_comm_unique_id(char* out128);
int knp_comm_init(knp_ctx* ctx, int rank, int nranks, const char* id128);
/* Optional second communicator (its own unique id) + stream for the halo exchanges, so that the exchange of an apply's input
 * overlaps the launch over the interior cells; knp_set_interior declares how many leading owned cells have no ghost neighbour
 * (checked).  Without these two calls every exchange runs on the context's stream in front of the apply. */
int knp_comm_init_halo(knp_ctx* ctx, const char* id128);
/* Instead of knp_comm_init: a host-staged communicator through the POSIX shared-memory segment `name` for ranks that are processes
 * of one node and may share one GPU (RCCL refuses that).  Same semantics -- summed / maximised reductions in rank order, peer halo
 * exchange -- with every transfer staged through the host: a validation path (the partitioned solver with 2-4 ranks on a one-GPU
 * box, tests/test_gpu_multirank.py), never the measured one.  red_doubles / out_doubles: capacity of a rank's reduction slot and
 * halo outbox.  Call knp_halo_tables afterwards (it publishes where each peer finds its message and ends in a barrier). */
int knp_comm_init_shm(knp_ctx* ctx, int rank, int nranks, const char* name, int64_t red_doubles, int64_t out_doubles);
int knp_set_interior(knp_ctx* ctx, int64_t n_interior);
/* send_cells: owned cell ids whose DoFs peer p needs, grouped by peer; ghosts of peer p occupy
 * cells [recv_offsets[p], recv_offsets[p]+recv_counts[p]). */
int knp_halo_tables(knp_ctx* ctx, int npeers, const int32_t* peers, const int64_t* send_counts,
                    const int32_t* send_cells, const int64_t* recv_offsets, const int64_t* recv_counts);
int knp_halo_exchange(knp_ctx* ctx, int field);
/* Sum of n <= 56 host scalars over the ranks of a partitioned run (one ncclAllReduce on the solver's stream; every rank receives the
 * same bits); leaves the values untouched without a communicator.  The host side uses it where a quantity that steers the solve
 * must be the SAME on all ranks: the step-0 residual target of the EMI solve (the reference gets this from PETSc's VecNorm over
 * the MPI communicator, src/knpemidg/solver.py:505-509) and the timings of the smoother selection (knpemidg/solver.py). */
int knp_allreduce_sum(knp_ctx* ctx, double* values, int n);

#ifdef __cplusplus
}
#endif
#endif
