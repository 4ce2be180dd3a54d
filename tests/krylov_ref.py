"""Host reference of the device Krylov solves' stopping tests (csrc/krylov.hip): the oracle's EMI / KNP matrices, the cell-block-Jacobi
inverses in the device's fp32 storage, the norms the device reports recomputed with exact-rounding sums, and a numpy replica of the
PCG scalar recurrence and its stopping test.  Test infrastructure only."""
import math

import numpy as np

import knpemi_oracle as ko

KNP_D8_FACTOR = 20.0            # solve.hip: knp_knp_solve scales rtol of the order-8 density test by this


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


class Ref:
    """Matrices, loads and preconditioner of an oracle Problem in the device's layout (cell-major, nd dofs per cell)."""

    def __init__(self, pb):
        self.pb, self.nd = pb, pb.nd
        self.nc = pb.mesh.num_cells()
        # 1 / vol stored in fp32 (context.hip: knp_ctx_create, `ivol`)
        self.w = (1.0 / pb.geom.vol).astype(np.float32).astype(np.float64)
        self.A_emi, self.b_emi, _ = ko.assemble_emi(pb, want_B=False)
        self.A_emi = self.A_emi.tocsr()
        self.binv_emi = block_inverses(self.A_emi, self.nd)
        self._phi_star = None

    # ---- norms of a residual / load vector r [ndof] --------------------------------------------------------------------------
    def norm_w2(self, r):
        """cell-volume-weighted 2-norm sqrt(sum_K |r_K|^2 / vol_K) (KNP_KNP_NORM2=1)"""
        rk = np.asarray(r, dtype=np.float64).reshape(self.nc, self.nd)
        return math.sqrt(_fsum((rk * rk).sum(axis=1) * self.w))

    def norm_d8(self, r):
        """order-8 norm of the density (sum_K (|r_K| / vol_K)^8)^(1/8), scaled to avoid under- / overflow of the 8th powers"""
        rk = np.asarray(r, dtype=np.float64).reshape(self.nc, self.nd)
        q = np.sqrt((rk * rk).sum(axis=1)) * self.w
        m = q.max()
        if m == 0.0:
            return 0.0
        return m * _fsum((q / m) ** 8) ** 0.125

    def norm_pc(self, binv, r):
        """PETSc's preconditioned norm ||M^-1 r|| (block-Jacobi M)"""
        z = apply_blocks(binv, r)
        return math.sqrt(_fsum(z * z))

    # ---- EMI ------------------------------------------------------------------------------------------------------------------
    def phi_star(self):
        """direct solve of the (singular, consistent) EMI system; leaves pb.phi as it was"""
        if self._phi_star is None:
            keep = self.pb.phi.copy()
            self._phi_star = ko.solve_emi(self.pb, direct=True).ravel().copy()
            self.pb.phi = keep
        return self._phi_star

    def solve_emi(self, b):
        """direct solve of A phi = b for another (consistent up to its mean) load, e.g. the device's B_EMI; mean-free phi"""
        import scipy.sparse.linalg as spla
        n = self.A_emi.shape[0]
        b = np.asarray(b, dtype=np.float64).ravel()
        b = b - b.mean()
        lu = spla.splu(self.A_emi.tocsc()[:n - 1, :n - 1], permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0,
                       options=dict(SymmetricMode=True))
        x = np.concatenate([lu.solve(b[:n - 1]), [0.0]])
        return x - x.mean()

    def energy(self, x):
        x = np.asarray(x, dtype=np.float64).ravel()
        return math.sqrt(max(_fsum(x * (self.A_emi @ x)), 0.0))

    def energy_error(self, phi, star=None):
        """relative energy-norm error ||phi - phi*||_A / ||phi*||_A (a constant shift is in the null space of A)"""
        star = self.phi_star() if star is None else star
        e = np.asarray(phi, dtype=np.float64).ravel() - star
        return self.energy(e) / self.energy(star)

    # ---- KNP ------------------------------------------------------------------------------------------------------------------
    def knp(self, k):
        """(A_knp, b_knp) of solved species k at the problem's current state"""
        return ko.assemble_knp(self.pb, k).tocsr(), ko.knp_rhs(self.pb, k)


def block_inverses(A, nd):
    """inverses of the nd x nd cell-diagonal blocks of A, rounded to fp32 as the device stores them (bjreal = float)"""
    n = A.shape[0]
    Ab = A.tobsr(blocksize=(nd, nd))
    Ab.sort_indices()
    rowid = np.repeat(np.arange(n // nd), np.diff(Ab.indptr))
    sel = Ab.indices == rowid
    diag = np.zeros((n // nd, nd, nd))
    diag[rowid[sel]] = Ab.data[sel]
    return np.linalg.inv(diag).astype(np.float32).astype(np.float64)


def apply_blocks(binv, r):
    nb, nd, _ = binv.shape
    return np.einsum("bij,bj->bi", binv, np.asarray(r, dtype=np.float64).reshape(nb, nd)).ravel()


def pcg(ref, rtol, r_abs, x0=None, maxit=20000, rule="device", precond=None, iters=None, dtype=np.float64):
    """Replica of the device PCG (krylov.hip: pcg_impl, scalar_op OP_CG_*) with block-Jacobi only and r_abs > 0 (error-controlled stop).
    rule "device": the stopping test of csrc/krylov.hip (cg_converged, OP_CG_BETA: smoothed decay rate); "onestep": the one-term
    extrapolation it replaced (alpha_k rho_{k+1} / (1 - min(beta_k, 0.9))).  Returns (x, iterations).
    precond: z = precond(r) instead of the cell blocks (amg_ref.EmiPrecond).  iters: exactly that many iterations, no stopping test
    (what the device returns for maxit = iters and a tolerance it cannot reach), in `dtype` (float64, np.longdouble, or "fsum":
    float64 with exactly rounded row sums)."""
    if iters is not None:
        return _pcg_fixed(ref, x0, precond, iters, dtype), iters
    A, b, binv = ref.A_emi, ref.b_emi, ref.binv_emi
    if precond is None:
        def precond(r):
            return apply_blocks(binv, r)
    x = np.zeros(A.shape[0]) if x0 is None else np.asarray(x0, dtype=np.float64).ravel().copy()
    w = A @ x
    r = b - w                                                           # k_cg_init
    z = precond(r)
    p = z.copy()
    st = dict(rho=float(z @ r), res=math.sqrt(z @ z), bnorm=math.sqrt(np.sum(precond(b) ** 2)),
              rnorm=ref.norm_d8(r), xa=max(float(x @ w), 0.0), sum=0.0, est=1e300, lb=0.0)
    if cg_converged(st, r_abs, rtol, 0):
        return x, 0
    for it in range(1, maxit + 1):
        w = A @ p
        pw = float(p @ w)
        alpha = st["rho"] / pw                                          # OP_CG_ALPHA
        st["sum"] += alpha * st["rho"]
        x += alpha * p                                                  # k_cg_update
        r -= alpha * w
        z = precond(r)
        rz = float(r @ z)                                               # OP_CG_BETA
        beta = rz / st["rho"]
        if rule == "onestep":
            q = min(max(beta, 0.0), 0.9)
        else:                                                           # decay rate smoothed over the last quarter of the steps
            lam = 1.0 / max(1.0, 0.25 * it)
            lb = math.log(max(beta, 1e-300))
            st["lb"] = lb if it == 1 else (1.0 - lam) * st["lb"] + lam * lb
            q = min(math.exp(st["lb"]), 0.999)
        st["est"] = math.sqrt(max(alpha * rz, 0.0) / (1.0 - q))
        st["rho"], st["res"], st["rnorm"] = rz, math.sqrt(z @ z), ref.norm_d8(r)
        if cg_converged(st, r_abs, rtol, it):
            return x, it
        p = z + beta * p                                                # k_cg_p
    raise RuntimeError("replica PCG did not converge")


def _pcg_fixed(ref, x0, precond, iters, dtype):
    """the vector recurrence of pcg_impl alone, `iters` times, in the working precision `dtype`"""
    if dtype == "fsum":
        import amg_ref
        wd, A = np.float64, amg_ref._FsumCsr(ref.A_emi)
    else:
        wd, A = dtype, ref.A_emi.astype(dtype)
    b = np.asarray(ref.b_emi).astype(wd)
    if precond is None:
        binv = ref.binv_emi.astype(wd)

        def precond(r):
            return np.einsum("bij,bj->bi", binv, r.reshape(binv.shape[0], -1)).ravel()
    x = np.zeros(A.shape[0], dtype=wd) if x0 is None else np.asarray(x0).astype(wd).ravel().copy()
    r = b - A @ x
    z = precond(r)
    p = z.copy()
    rho = z @ r
    for _ in range(iters):
        w = A @ p
        alpha = rho / (p @ w)
        x = x + alpha * p
        r = r - alpha * w
        z = precond(r)
        rz = r @ z
        p = z + (rz / rho) * p
        rho = rz
    return x


def cg_converged(st, r_abs, rtol, it):
    """krylov.hip: cg_converged, residual-target branch"""
    if st["res"] <= 1e-11 * st["bnorm"]:
        return True
    return it > 0 and st["rnorm"] <= r_abs and st["est"] <= rtol * math.sqrt(max(st["xa"], st["sum"]))
