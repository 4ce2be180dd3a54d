"""Host model of what one linear solve hands the next (csrc/solve.hip: PrecState, Fields; csrc/context.hip: knp_upload, knp_set_params)
-- test infrastructure, beside krylov_ref.py / amg_ref.py.

`Model` is driven by the events the device sees -- `upload(field)`, `set_params()`, `set_emi_dg_smoother()`, `solve(...)` /
`done(...)`, the environment switches as constructor arguments -- and answers, per system ("emi" / "knp"): the initial guess of the next
solve, what h1, h2 and nh hold afterwards, from which coefficient state the per-cell block inverses in use were built and their age,
whether the solve re-estimates the spectral bound of the Chebyshev cell-block smoother and on which matrix, blocks and right-hand side,
and lmax_age / it_ref afterwards.  The rules are written from the text of solve.hip and context.hip:

  extrapolate_guess   on unless KNP_EXTRAPOLATE says otherwise (0 none, 2 EMI only, 3 KNP only) or splitting == 2;
                      nh = 0: x kept; nh = 1 or order 1: 2 x - h1; nh = 2 and order 2: 3 (x - h1) + h2; then h2 <- h1 if order 2 or
                      KNP_FUSE_EXTRAP=0 (read per call), h1 <- x, nh <- min(nh + 1, 2)
  knp_upload          C, C_ELIM, PHI, KAPPA: reset_lagged (both ages 0, both bounds missing); PHI: emi.nh = 0; C: knp.nh = 0
  knp_set_params      reset_lagged; the class table is rebuilt by the next KNP solve (its scratch is the per-cell array); no history reset
  lagged_rebuild      age % KNP_BJ_LAG == 0: per-cell inverses from the CURRENT coefficients; ++age.  A KNP solve on the class table
                      sets age = 0 instead
  chebyshev_bound     estimate when the bound is missing, else when ++lmax_age >= 64, else when it_ref > 0 and 2 last_it > 3 it_ref + 2
                      (last_it: iterations of the previous solve of that system, converged or not); lmax = 1.1 lambda of 20 power
                      iterations from b on this solve's matrix with the blocks in use; lmax_age = 0, it_ref = -1
  note_iterations     after a CONVERGED solve: it_ref < 0 -> it_ref = its iteration count
  block-set flip      (KNP) bound missing, it_ref = 0

`mut`: one deliberate error (MUTATIONS); tests/test_solve_state_ref_host.py shows that each one changes a prediction on the sequences
the device runs (tests/test_gpu_solve_state.py).  A coefficient state is whatever hashable label the caller gives it."""
import numpy as np

RESET_FIELDS = ("C", "C_ELIM", "PHI", "KAPPA")
MUTATIONS = ("guess_is_previous", "guess_3x_2h1", "h1_not_rotated", "history_kept_by_upload", "history_dropped_by_set_params",
             "lag_7", "lag_9", "rebuild_every_solve", "age_kept_by_upload", "bound_without_1.1", "bound_every_solve",
             "bound_never_at_64", "jump_rule_ge")
# the 18 solves of the lagged-inverse sequences: index of the coefficient state before every solve.  Neighbours differ, and so do the
# states at the solves where the rules and the broken rules rebuild (0, 7, 8, 9, 11, 14, 16).
LAG_STATES = (0, 1, 2, 3, 0, 1, 2, 3, 1, 2, 3, 0, 1, 2, 3, 0, 2, 1)
LAG_EVENTS = {11: "set_params", 14: "upload C_ELIM"}


class System:
    def __init__(self, emi):
        self.emi = emi
        self.nh, self.h1, self.h2 = 0, None, None
        self.age, self.built = 0, None                  # `built`: state label the per-cell array was last built from
        self.lmax, self.lmax_age, self.it_ref, self.last_it = None, 0, 0, 0

    def counters(self):
        return dict(nh=self.nh, age=self.age, lmax_age=self.lmax_age, it_ref=self.it_ref)


class Model:
    def __init__(self, extrapolate=1, order_emi=1, order_knp=1, bj_lag=8, splitting=1, table=False, mut=None):
        assert mut is None or mut in MUTATIONS
        self.mode, self.order, self.splitting, self.mut = int(extrapolate), dict(emi=int(order_emi), knp=int(order_knp)), splitting, mut
        self.lag = {"lag_7": 7, "lag_9": 9, "rebuild_every_solve": 1}.get(mut, bj_lag if bj_lag > 0 else 1)
        self.emi, self.knp = System(True), System(False)
        self.table = 0 if table else -1                 # bj_tab_state: 0 not built, 1 ready, -1 unavailable
        self.used_tab = -1
        self.emi_cheb = None

    @classmethod
    def from_env(cls, env, **kw):
        """the switches solve.hip reads once per process, from an environment dict"""
        oa = int(env.get("KNP_EXTRAPOLATE_ORDER", 0))
        return cls(extrapolate=int(env.get("KNP_EXTRAPOLATE", 1)), order_emi=int(env.get("KNP_EXTRAPOLATE_ORDER_EMI", oa or 1)),
                   order_knp=int(env.get("KNP_EXTRAPOLATE_ORDER_KNP", oa or 1)), bj_lag=int(env.get("KNP_BJ_LAG", 8)), **kw)

    def sys(self, name):
        return {"emi": self.emi, "knp": self.knp}[name]

    # ---- events ----------------------------------------------------------------------------------------------------------------
    def reset_lagged(self):
        for s in (self.emi, self.knp):
            s.age, s.lmax = 0, None

    def upload(self, field):
        if field in RESET_FIELDS:
            if self.mut == "age_kept_by_upload":
                self.emi.lmax = self.knp.lmax = None
            else:
                self.reset_lagged()
        if self.mut != "history_kept_by_upload":
            if field == "PHI":
                self.emi.nh = 0
            if field == "C":
                self.knp.nh = 0

    def set_params(self, splitting=None):
        self.reset_lagged()
        if self.table != -1:
            self.table = 0
        if splitting is not None:
            self.splitting = splitting
        if self.mut == "history_dropped_by_set_params":
            self.emi.nh = self.knp.nh = 0

    def set_emi_dg_smoother(self, cheb):
        if cheb != self.emi_cheb:
            self.emi.lmax = None
        self.emi_cheb = cheb

    def solve(self, name, x, state, b=None, cheb=True, use_tab=False, keep_h2=False):
        """the part of knp_emi_solve / knp_knp_solve in front of the Krylov loop.  x: the field the solve starts from; state: label of
        the coefficients (and matrix) of this solve; b: label of its right-hand side; cheb: the solve runs the Chebyshev cell-block
        smoother; use_tab: (KNP) it runs on the class table; keep_h2: KNP_FUSE_EXTRAP=0 at this call.
        Returns dict(guess, blocks: label the blocks in use were built from ("table": the drift-free class table), rebuilt, estimate,
        lmax: what the bound in use was estimated on -- dict(matrix, blocks, b, factor) -- or None without the smoother)."""
        s = self.sys(name)
        rebuilt = False
        if not s.emi:
            if self.table == 0:                          # build_bj_table: the per-cell array is its scratch
                self.table, s.built = 1, "drift-free"
            use_tab = bool(use_tab) and self.table == 1
            if int(use_tab) != self.used_tab:
                s.lmax, s.it_ref, self.used_tab = None, 0, int(use_tab)
        if use_tab:
            s.age = 0
        else:
            if s.age % self.lag == 0:
                s.built, rebuilt = state, True
            s.age += 1
        guess = self._extrapolate(s, np.asarray(x, dtype=np.float64), keep_h2)
        estimate = False
        if cheb:
            jump = (lambda a, r: a >= r) if self.mut == "jump_rule_ge" else (lambda a, r: a > r)
            missing = s.lmax is None
            aged = False
            if not missing:
                s.lmax_age += 1
                aged = s.lmax_age >= 64 and self.mut != "bound_never_at_64"
            if missing or aged or (s.it_ref > 0 and jump(2 * s.last_it, 3 * s.it_ref + 2)) or self.mut == "bound_every_solve":
                s.lmax = dict(matrix=state, blocks="table" if use_tab else s.built, b=b,
                              factor=1.0 if self.mut == "bound_without_1.1" else 1.1)
                s.lmax_age, s.it_ref, estimate = 0, -1, True
        return dict(guess=guess, blocks="table" if use_tab else s.built, rebuilt=rebuilt, estimate=estimate, lmax=s.lmax if cheb else None)

    def done(self, name, converged, niter):
        """behind the Krylov loop: niter = the iteration count the device reports (KNP: the largest of the species)"""
        s = self.sys(name)
        s.last_it = int(niter)
        if converged and s.it_ref < 0:
            s.it_ref = int(niter)

    def _extrapolate(self, s, x, keep_h2):
        order = self.order["emi" if s.emi else "knp"]
        on = self.mode == 1 or (self.mode == 2 and s.emi) or (self.mode == 3 and not s.emi)
        if not on or self.splitting == 2:
            return x
        if s.h1 is None:
            s.h1, s.h2 = np.zeros_like(x), np.zeros_like(x)
        if s.nh >= 2 and order >= 2:
            g = 3.0 * (x - s.h1) + s.h2
        elif s.nh >= 1:
            g = {"guess_is_previous": lambda: x.copy(), "guess_3x_2h1": lambda: 3.0 * x - 2.0 * s.h1}.get(self.mut, lambda: 2.0 * x - s.h1)()
        else:
            g = x
        if order >= 2 or keep_h2:
            s.h2 = s.h1.copy()
        if not (self.mut == "h1_not_rotated" and s.nh >= 1):
            s.h1 = x.copy()
        if s.nh < 2:
            s.nh += 1
        return g


def order2_bound(x, h1, h2):
    """per entry: 2 ulp of the largest of the three terms of 3 x - 3 h1 + h2 (contraction may change the last bit)"""
    return 2.0 * np.spacing(np.maximum(np.maximum(np.abs(3.0 * x), np.abs(3.0 * h1)), np.abs(h2)))


# ---- cell blocks ----------------------------------------------------------------------------------------------------------------
def cell_blocks(A, nd):
    """the nd x nd cell-diagonal blocks of A [nc, nd, nd] (float64, not inverted)"""
    n = A.shape[0]
    Ab = A.tobsr(blocksize=(nd, nd))
    Ab.sort_indices()
    rowid = np.repeat(np.arange(n // nd), np.diff(Ab.indptr))
    sel = Ab.indices == rowid
    diag = np.zeros((n // nd, nd, nd))
    diag[rowid[sel]] = Ab.data[sel]
    return diag


def gauss_jordan_inverse(B, dtype=np.longdouble):
    """inverses of the blocks B [nb, n, n] by Gauss-Jordan elimination with partial pivoting in `dtype`, all blocks at once"""
    B = np.asarray(B)
    nb, n, _ = B.shape
    M = np.concatenate([B.astype(dtype), np.broadcast_to(np.eye(n, dtype=dtype), (nb, n, n))], axis=2)
    ar = np.arange(nb)
    for k in range(n):
        p = k + np.argmax(np.abs(M[:, k:, k]), axis=1)
        rk, rp = M[ar, k].copy(), M[ar, p].copy()
        M[ar, k], M[ar, p] = rp, rk
        M[:, k] = M[:, k] / M[:, k, k][:, None]
        f = M[:, :, k].copy()
        f[:, k] = 0
        M = M - f[:, :, None] * M[:, k][:, None, :]
    return M[:, :, n:]


def block_reference(B, fp32=False):
    """(inv64 [nb, n, n], bound [nb]) of the blocks B: numpy's float64 inverse and, per block, one fp32 ulp of its largest entry plus
    32 times the distance of the float64 inverse from the extended-precision one -- from the reference alone.
    fp32: also the inverses as an fp32 array holds them, rounded from the EXTENDED-precision inverse (as float64 values): the float64
    inverse rounds a few entries in 10^5 the other way, where its own error straddles an fp32 rounding boundary, and an iterate
    computed with such a block is hundreds of its bounds away"""
    inv64 = np.linalg.inv(B)
    hp = gauss_jordan_inverse(B)
    big = np.abs(inv64).max(axis=(1, 2))
    err = np.abs(inv64 - hp).max(axis=(1, 2)).astype(np.float64)
    out = inv64, 2.0 ** -23 * big + 32.0 * err
    return out + (hp.astype(np.float32).astype(np.float64),) if fp32 else out


def lambda_bound(lam64, lam_hp):
    """comparison bound of a spectral bound: 32 times the float64 replica's distance from the extended-precision one, at least 1e-13"""
    return max(32.0 * abs(float(lam64) - float(lam_hp)), 1e-13 * abs(float(lam_hp)))


def lambda_max(As, binvs, bs, dtype=np.float64, factor=1.1, iters=20):
    """amg_ref.bj_lambda_max in a working precision (krylov.hip: bj_lambda_max_impl, times `factor`, the 1.1 of solve.hip)"""
    A = [M.astype(dtype) for M in As]
    Bi = [np.asarray(b).astype(dtype) for b in binvs]
    v = [np.asarray(b).astype(dtype).ravel().copy() for b in bs]
    blocks = lambda binv, r: np.einsum("bij,bj->bi", binv, r.reshape(binv.shape[0], -1)).ravel()
    nv = max(np.abs(x).max() for x in v)
    lam = dtype(0)
    for _ in range(iters):
        y = [blocks(b, M @ x) for M, b, x in zip(A, Bi, v)]
        ny = max(np.abs(x).max() for x in y)
        lam = ny / nv
        v = [(1 / ny) * x for x in y]
        nv = dtype(1)
    return dtype(factor) * lam
