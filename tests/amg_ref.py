"""Host replica of the auxiliary-space preconditioner (csrc/amg_vcycle.hip, csrc/amg_restrict.hip, csrc/krylov.hip) -- test infrastructure.

  * `store`: a knpemidg.amg-style hierarchy as the device stores it -- CSR values of A, P, R and the coarse (pseudo-)inverse rounded to
    fp32 (amg_upload.hip: up_csr, amg_finish_impl), dinv / rho / cheb_lower in fp64 -- converted to a working precision: float64, or
    np.longdouble where that has a 64-bit mantissa (`HP`; elsewhere the high-precision run sums its rows with math.fsum).
  * `vcycle`: amg_vcycle_eager, level by level, for [ncol, n] right-hand sides (the columns are independent).
  * `EmiPrecond` / `KnpPrecond`: the two-level preconditioners of pcg_impl / bicgstab_impl around it; `bj_lambda_max`.
  * `bicgstab`: k iterations in the form of bicgstab_impl (the PCG twin is krylov_ref.pcg with `precond` / `iters`).
  * `gmres` / `gmres_free`: restarted GMRES in the form of gmres_impl / gm_scalar_op -- k iterations, or to convergence by the device's
    rules with the distance of every decision from its threshold; GM_CASES / GM_FREE_CASES: what the device is compared on.
  * `launches`: which (kernel, G, NC) instantiations a hierarchy reaches (amg_vcycle.hip: by_density).
  * `synthetic`: seeded hand-built hierarchies (any density, any level size) for tests/test_amg_ref_host.py and a comparison on the device.
  * `Dist0` / `vcycle_dist0`: level 0 in the row-distributed form of a partitioned run (amg_vcycle_dist0, interface_accumulate) -- `store`,
    `emi_xk` and `knp_xk` take it as `dist=`; DIST_MUTATIONS: its deliberate errors; PART_GROUPS: what the partitioned device is compared on.
A `mut = (name, level)` argument applies one deliberate error (MUTATIONS; drop_tail: (name, (level, matrix))) -- the CPU tests show
that each one is far above the comparison bound (`bound`).
The "fsum" fallback is NOT a wider arithmetic: only the row sums of the matrix products are exactly rounded, the vector updates, inner
products and cell-block products stay float64 (measured on a three-level V-cycle: 2.2e-15 from the long-double result against 3.0e-15
for plain float64).  Where long double has no 64-bit mantissa, `bound` therefore rests on its 1e-13 floor rather than on a measured
rounding error; on x86-64, where the tests run, HP is the 80-bit long double."""
import math

import numpy as np
import scipy.sparse as sp

HP = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else None

# average-row-length limits of by_density (csrc/amg_vcycle.hip; the second one is g4_limit(), KNP_AMG_G4)
BANDS = ((12.0, 1), (40.0, 4), (96.0, 8), (math.inf, 64))
KERNELS = ("k_csr<0>", "k_csr<1>", "k_csr<2>", "k_csr_first", "k_cheb_first_res", "k_cheb_step")
MUTATIONS = ("no_round_A", "drop_tail", "swap_columns", "short_post_smooth", "no_prolongation", "dense_last_row")


# ions of the KNP cases by number of solved species (None: the K / Cl / Na problem), and the cases the device runs on the drift-free
# class table of solve.hip (tests/test_gpu_amg.py) -- (mesh, solved species, hierarchy or one per species, four materials) at the
# potential TABLE_PHI_SCALE times the synthetic one; tests/test_amg_ref_host.py asserts that the replica supports every one of them
IONS = {2: None, 3: ("K", "Cl", "X", "Na"), 4: ("K", "Cl", "X", "Y", "Na")}
TABLE_PHI_SCALE = 0.05
TABLE_CASES = (("box_P1", 2, "bands", False), ("box_P1", 2, "bands_t0", False), ("box_P1", 2, "coarse_257", False),
               ("box_P1", 2, "bands", True), ("box_P1", 3, "bands", False), ("box_P1", 4, "bands", False),
               ("box_P1", 2, ("bands", "mid"), True),
               ("box_P2", 2, "bands", False), ("box_P2", 2, "coarse_257", False), ("box_P2", 2, "bands_t0", True))


class _Level:
    pass


def band_G(M):
    avg = M.nnz / M.shape[0] if M.shape[0] else 0.0
    return next(g for lim, g in BANDS if avg <= lim)


def _unroll(ncol):
    return 2 if ncol % 2 == 0 else 4                    # row_dot: (col, val) pairs in flight per lane


class _FsumCsr:
    """float64 matrix whose products sum every row with math.fsum (the high-precision run where long double is no wider)"""

    def __init__(self, M):
        self.M = sp.csr_matrix(M)
        self.shape = self.M.shape

    def __matmul__(self, x):
        M, out = self.M, np.zeros(self.shape[0])
        for i in range(self.shape[0]):
            k = slice(M.indptr[i], M.indptr[i + 1])
            out[i] = math.fsum((M.data[k] * x[M.indices[k]]).tolist())
        return out


def _drop_tail(M, ncol):
    """mutation: the last entry of every row whose length is 1 modulo U * G is lost"""
    M = M.tocsr().copy()
    M.sort_indices()
    m = _unroll(ncol) * band_G(M)
    ln = np.diff(M.indptr)
    hit = np.nonzero(ln % m == 1)[0]
    M.data[M.indptr[hit + 1] - 1] = 0.0
    return M, len(hit)


def store(levels, dtype=np.float64, mut=None, ncol=1, dist=None):
    """device storage of `levels` (objects with A, dinv, rho, cheb_degree, cheb_lower, P, R; the last one with pinv) in `dtype`.
    dist = a `Dist0`: level 0 also in the row-distributed form of a partitioned run, every rank's rows as the device stores them
    (`vcycle_dist0`); or (`Dist0`, level-0 matrices of the ranks) for other matrices than Dist0Space.localize's split of the global one"""
    fsum = dtype == "fsum"
    wd = np.float64 if fsum else dtype
    name, ml = mut if mut else (None, -1)
    out, dropped = [], 0
    for l, lv in enumerate(levels):
        L = _Level()
        L.n = lv.A.shape[0]
        L.cheb_degree = int(lv.cheb_degree)
        L.dinv = np.asarray(lv.dinv, dtype=np.float64).astype(wd)
        L.rho, L.cheb_lower = wd(lv.rho), wd(lv.cheb_lower)
        mats = {"A": lv.A}
        if l < len(levels) - 1:
            mats.update(P=lv.P, R=lv.R)
        for key, M in mats.items():
            M = sp.csr_matrix(M, dtype=np.float64)
            M.sort_indices()
            if not (name == "no_round_A" and l == ml and key == "A"):
                M = sp.csr_matrix((M.data.astype(np.float32).astype(np.float64), M.indices, M.indptr), shape=M.shape)
            if name == "drop_tail" and (l, key) == tuple(ml):                       # ml = (level, "A" | "P" | "R")
                M, k = _drop_tail(M, ncol)
                dropped += k
            setattr(L, key, _FsumCsr(M) if fsum else M.astype(wd))
        out.append(L)
    assert name != "drop_tail" or dropped, "drop_tail: no row of length 1 modulo U * G"
    pinv = np.asarray(levels[-1].pinv).astype(np.float32).astype(np.float64)
    out[-1].pinv = _FsumCsr(pinv) if fsum else pinv.astype(wd)
    if dist is not None:
        d0, A_local = dist if isinstance(dist, tuple) else (dist, [None] * dist.world)
        assert len(levels) >= 2, "a distributed level 0 needs a coarser level"
        out[0].dist0, out[0].ranks = d0, []
        for d, Ar in zip(d0.D, A_local):
            lv, L = d.localize(levels, Ar)[0], _Level()
            L.n, L.dinv = lv.A.shape[0], np.asarray(lv.dinv, dtype=np.float64).astype(wd)
            for key in ("A", "P", "R"):
                M = sp.csr_matrix(getattr(lv, key), dtype=np.float64)
                M.sort_indices()
                M = sp.csr_matrix((M.data.astype(np.float32).astype(np.float64), M.indices, M.indptr), shape=M.shape)
                setattr(L, key, _FsumCsr(M) if fsum else M.astype(wd))
            out[0].ranks.append(L)
    return out


def smooth(L, x, b, zero_guess, steps=None):
    """amg_vcycle.hip: smooth() / amg.hpp: Cheb -- Chebyshev polynomial of D^-1 A on [cheb_lower * rho, rho]"""
    lmax, lmin = L.rho, L.cheb_lower * L.rho
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    steps = L.cheb_degree if steps is None else steps
    if steps < 1:
        return x
    r = b.copy() if zero_guess else b - L.A @ x
    d = L.dinv * r * (1 / theta)                                        # k_cheb_first / k_cheb_first_res / k_csr_first
    x = d.copy() if zero_guess else x + d
    for _ in range(1, steps):                                           # k_cheb_step
        rho_new = 1 / (2 * sigma - rho)
        r = r - L.A @ d
        d = (rho_new * rho) * d + (2 * rho_new / delta) * L.dinv * r
        x = x + d
        rho = rho_new
    return x


def _vcycle_levels(H, B, l, mut):
    """B: list of the columns' right-hand sides on level l"""
    L = H[l]
    name, ml = mut if mut else (None, -1)
    here = l == ml
    if name == "drop_tail":
        here = False                                                    # (applied by `store`)
    if l == len(H) - 1:                                                 # k_dense_mv
        X = [L.pinv @ b for b in B]
        if here and name == "dense_last_row":
            for x in X:
                x[-1] = 0
    elif L.cheb_degree == 0:                                            # transfer-only level
        Xc = _vcycle_levels(H, [L.R @ b for b in B], l + 1, mut)
        X = [L.P @ xc for xc in Xc]
        if here and name == "no_prolongation":
            X = [0 * x for x in X]
    else:
        X = [smooth(L, None, b, True) for b in B]
        Xc = _vcycle_levels(H, [L.R @ (b - L.A @ x) for b, x in zip(B, X)], l + 1, mut)
        if not (here and name == "no_prolongation"):
            X = [x + L.P @ xc for x, xc in zip(X, Xc)]
        post = L.cheb_degree - 1 if here and name == "short_post_smooth" else None
        X = [smooth(L, x, b, False, post) for x, b in zip(X, B)]
    if here and name == "swap_columns":
        assert len(X) >= 2, "swap_columns needs two right-hand-side columns"
        X[0], X[1] = X[1], X[0]
    return X


# ---- the row-distributed level 0 of a partitioned run (csrc/amg_vcycle.hip: amg_vcycle_dist0; csrc/comm.hip: interface_accumulate) ----
# deliberate errors of the distributed form (mut = (name, 0)): the third and later owners of a shared dof left out of its sum; A d of
# the extra Chebyshev steps not accumulated; the zero-guess smoother on the un-accumulated b; the last rank's part missing from the
# level-1 right-hand side; a message read as [column][position] instead of [position][column]; a peer's message read at the offset
# of that peer's message to another rank
DIST_MUTATIONS = ("two_owners", "no_step_accumulation", "zero_guess_unaccumulated", "rank_missing_level1", "message_interleave",
                  "peer_offset")


class Dist0:
    """The finest conforming level of `host` in the row-distributed form of the cell partition `owner` [nc]: per rank the rows
    (knpemidg.amg.Dist0Space), the shared-dof tables the device gets (interface_tables), the owned cells and the DG <-> conforming
    maps of those cells; `emi_matrices`: the ranks' EMI level-0 matrices assembled from their own elements
    (Dist0Space.local_matrix), which the device does NOT run on (their fp32 roundings do not add up to the rounded global matrix)."""

    def __init__(self, host, owner):
        from knpemidg import amg
        self.host, self.owner = host, np.asarray(owner)
        self.world = int(self.owner.max()) + 1
        mesh, surf = host.mt[0], np.asarray(host.mt[2].array())
        space = host.cs2 or host.cs
        mem = np.nonzero((mesh.facet_cells[:, 1] >= 0) & np.isin(surf, [1]))[0]
        self.D = [amg.Dist0Space(space, self.owner, mem, r, self.world) for r in range(self.world)]
        self.tabs = [d.interface_tables() for d in self.D]
        self.cells = [np.nonzero(self.owner == r)[0] for r in range(self.world)]
        nd = host.nd
        # DG dofs of the owned cells (positions in a global DG vector) and their conforming dofs in the rank's numbering
        self.dg = [(c[:, None] * nd + np.arange(nd)[None, :]).ravel() for c in self.cells]
        self.cg = [d.local_dg2cg(c).ravel() for d, c in zip(self.D, self.cells)]
        # per rank: the concatenated send list, and per peer (offset, length) of the message to it
        self.send_idx = [np.concatenate(t[1]) if t[0] else np.zeros(0, dtype=np.int64) for t in self.tabs]
        self.send_off = [np.concatenate([[0], np.cumsum([len(l) for l in t[1]])]).astype(np.int64) for t in self.tabs]
        self._emi = None

    def owners(self):
        """number of ranks that hold every conforming dof"""
        cnt = np.zeros(self.D[0].space.n, dtype=np.int64)
        for d in self.D:
            cnt[d.verts] += 1
        return cnt

    def emi_matrices(self):
        """the ranks' EMI level-0 matrices assembled from their own elements"""
        if self._emi is None:
            pb = self.host.pb
            self._emi = [d.local_matrix(pb.kappa(), membrane_C=float(pb.C_phi)) for d in self.D]
        return self._emi

    def transfers(self, dtype):
        """per rank (P_dg of the owned cells [owned DG dofs, rows], its transpose) in the working precision"""
        out = []
        for d, dg, cg in zip(self.D, self.dg, self.cg):
            Pd = sp.csr_matrix((np.ones(len(cg)), (np.arange(len(cg)), cg)), shape=(len(cg), d.n))
            out.append((_FsumCsr(Pd), _FsumCsr(Pd.T)) if dtype == "fsum" else (Pd.astype(dtype), Pd.T.tocsr().astype(dtype)))
        return out


def _accumulate(d0, V, mut=None):
    """interface_accumulate on V[column][rank]: every rank packs its values at the dofs it shares with each peer ([position][column]),
    reads the peers' messages, and replaces every shared dof by the sum over all its owners in ascending rank order"""
    ncol, name = len(V), (mut[0] if mut else None)
    send = [np.stack([V[j][r][idx] for j in range(ncol)], axis=1).ravel() for r, idx in enumerate(d0.send_idx)]
    out = [[None] * d0.world for _ in range(ncol)]
    for r, (peers, lists, uvtx, aptr, asrc) in enumerate(d0.tabs):
        if not peers:
            for j in range(ncol):
                out[j][r] = V[j][r]
            continue
        recv = []
        for q, l in zip(peers, lists):
            k = d0.tabs[q][0].index(r)
            if name == "peer_offset":                                   # the offset of q's message to its next peer
                k = (k + 1) % len(d0.tabs[q][0])
            off = min(int(d0.send_off[q][k]), len(d0.send_idx[q]) - len(l))
            recv.append(send[q][off * ncol:(off + len(l)) * ncol])
        recv = np.concatenate(recv)
        total = len(recv) // ncol
        aptr, asrc, uvtx = np.asarray(aptr, dtype=np.int64), np.asarray(asrc, dtype=np.int64), np.asarray(uvtx, dtype=np.int64)
        cnt = np.diff(aptr)
        if name == "two_owners":
            cnt = np.minimum(cnt, 2)
        for j in range(ncol):
            v = V[j][r]
            w = v.copy()
            s = np.zeros(len(uvtx), dtype=v.dtype)
            for t in range(int(cnt.max())):                             # the terms of every sum in the order of k_if_add
                on = np.nonzero(cnt > t)[0]
                src = asrc[aptr[on] + t]
                at = src + j * total if name == "message_interleave" else src * ncol + j
                s[on] = s[on] + np.where(src < 0, v[uvtx[on]], recv[np.where(src < 0, 0, at)])
            w[uvtx] = s
            out[j][r] = w
    return out


def _smooth_dist0(L, B, X, mut):
    """dist0_smooth: `smooth` on the ranks' rows -- B[column][rank] partial sums, X accumulated (None: zero guess); every product with
    a sub-assembled matrix is accumulated before it is used"""
    name = mut[0] if mut else None
    lmax, lmin = L.rho, L.cheb_lower * L.rho
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    ranks, nr = L.ranks, len(L.ranks)
    each = lambda f: [[f(j, r) for r in range(nr)] for j in range(len(B))]
    if X is None:
        R = each(lambda j, r: B[j][r].copy())
        if name != "zero_guess_unaccumulated":
            R = _accumulate(L.dist0, R, mut)
    else:
        R = _accumulate(L.dist0, each(lambda j, r: B[j][r] - ranks[r].A @ X[j][r]), mut)
    D = each(lambda j, r: ranks[r].dinv * R[j][r] * (1 / theta))
    X = each(lambda j, r: D[j][r].copy()) if X is None else each(lambda j, r: X[j][r] + D[j][r])
    for _ in range(1, L.cheb_degree):
        rho_new = 1 / (2 * sigma - rho)
        T = each(lambda j, r: ranks[r].A @ D[j][r])
        if name != "no_step_accumulation":
            T = _accumulate(L.dist0, T, mut)
        R = each(lambda j, r: R[j][r] - T[j][r])
        D = each(lambda j, r: (rho_new * rho) * D[j][r] + (2 * rho_new / delta) * ranks[r].dinv * R[j][r])
        X = each(lambda j, r: X[j][r] + D[j][r])
        rho = rho_new
    return X


def vcycle_dist0(H, B, mut=None):
    """amg_vcycle_dist0 (and restrict_tail for a transfer-only level 0): B[column][rank] the ranks' partial sums of the level-0
    right-hand side; returns X[column][rank], accumulated.  The level-1 right-hand side is the sum of the ranks' parts in rank order
    (the all-reduce), the levels below are the replicated ones (`_vcycle_levels`)."""
    L = H[0]
    name = mut[0] if mut else None
    ranks, nr = L.ranks, len(L.ranks)
    assert name is None or name in DIST_MUTATIONS
    part_of = range(nr - 1) if name == "rank_missing_level1" else range(nr)

    def allreduce(parts):
        s = parts[part_of[0]].copy()
        for r in part_of[1:]:
            s = s + parts[r]
        return s
    if L.cheb_degree == 0:
        Xc = _vcycle_levels(H, [allreduce([ranks[r].R @ b[r] for r in range(nr)]) for b in B], 1, None)
        return [[ranks[r].P @ xc for r in range(nr)] for xc in Xc]
    X = _smooth_dist0(L, B, None, mut)
    Xc = _vcycle_levels(H, [allreduce([ranks[r].R @ (b[r] - ranks[r].A @ x[r]) for r in range(nr)]) for b, x in zip(B, X)], 1, None)
    X = [[x[r] + ranks[r].P @ xc for r in range(nr)] for x, xc in zip(X, Xc)]
    return _smooth_dist0(L, B, X, mut)


def vcycle(H, B, mut=None):
    """x = V(b) for every row of B [ncol, n_0] (or one vector [n_0]); H from `store`"""
    B = np.asarray(B)
    if B.ndim == 1:
        return _vcycle_levels(H, [B], 0, mut)[0]
    return np.stack(_vcycle_levels(H, [b for b in B], 0, mut))


# ---- the two-level preconditioners of krylov.hip -------------------------------------------------------------------------------------
BJ_LMIN = 0.05                                                          # krylov.hip: bj_lmin_frac


def _blocks(binv, r):
    nb, nd, _ = binv.shape
    return np.einsum("bij,bj->bi", binv, r.reshape(nb, nd)).ravel()


def bj_lambda_max(As, binvs, bs, iters=20):
    """krylov.hip: bj_lambda_max_impl (the systems are normalised together: max over the species), times the 1.1 of solve.hip"""
    v = [np.asarray(b, dtype=np.float64).copy() for b in bs]
    nv = max(np.abs(x).max() for x in v)
    lam = 0.0
    for _ in range(iters):
        y = [_blocks(Bi, A @ x) for A, Bi, x in zip(As, binvs, v)]
        ny = max(np.abs(x).max() for x in y)
        lam = ny / nv
        a = 1.0 / ny
        v = [a * x for x in y]
        nv = 1.0
    return 1.1 * lam


def _cheb2_coefficients(lmax, wd):
    lmax = wd(lmax)
    lmin = wd(BJ_LMIN) * lmax
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    rho0 = 1 / sigma
    rho1 = 1 / (2 * sigma - rho0)
    return (1 + rho1 * rho0) / theta + 2 * rho1 / delta, (2 * rho1 / delta) / theta, theta       # cr, ctt, theta


class _TwoLevel:
    def __init__(self, A, binv, dg2cg, ncg, dtype):
        self.wd = np.float64 if dtype == "fsum" else dtype
        self.A = [_FsumCsr(M) if dtype == "fsum" else sp.csr_matrix(M).astype(self.wd) for M in A]
        self.binv = [np.asarray(b).astype(self.wd) for b in binv]
        d = np.asarray(dg2cg).ravel()
        Pd = sp.csr_matrix((np.ones(len(d)), (np.arange(len(d)), d)), shape=(len(d), ncg))
        self.Pd, self.Pdt = (Pd.astype(self.wd), Pd.T.tocsr().astype(self.wd)) if dtype != "fsum" else (_FsumCsr(Pd), _FsumCsr(Pd.T))
        self._dtype, self._tr = dtype, None

    def coarse(self, H, C, mut):
        """P_dg V(P_dg^T c) for the columns C [ncol, ndof] through the hierarchy H; with a row-distributed level 0 every rank restricts
        the DG dofs of its owned cells (partial sums), and prolongs its accumulated rows to them"""
        if not hasattr(H[0], "ranks"):
            return [self.Pd @ e for e in vcycle(H, np.stack([self.Pdt @ c for c in C]), mut)]
        d0 = H[0].dist0
        if self._tr is None:
            self._tr = d0.transfers(self._dtype)
        X = vcycle_dist0(H, [[Pt @ c[dg] for (_, Pt), dg in zip(self._tr, d0.dg)] for c in C], mut)
        out = []
        for x in X:
            z = np.zeros(len(C[0]), dtype=self.wd)
            for (P, _), dg, xr in zip(self._tr, d0.dg, x):
                z[dg] = P @ xr
            out.append(z)
        return out


class EmiPrecond(_TwoLevel):
    """pcg_impl: z = S(r) + P_dg V(P_dg^T r); S = the fp32 cell blocks (lmax = 0) or the two-step Chebyshev block-Jacobi (k_bj_cheb2)"""

    def __init__(self, A, binv, dg2cg, H, lmax=0.0, dtype=np.float64, mut=None):
        super().__init__([A], [binv], dg2cg, H[0].n, dtype)
        self.H, self.lmax, self.mut = H, lmax, mut

    def __call__(self, r):
        z = _blocks(self.binv[0], r)
        if self.lmax > 0.0:
            cr, ctt, _ = _cheb2_coefficients(self.lmax, self.wd)
            z = _blocks(self.binv[0], cr * r - ctt * (self.A[0] @ z))
        return z + self.coarse(self.H, [r], self.mut)[0]


class KnpPrecond(_TwoLevel):
    """bicgstab_impl, hybrid form: z_s = S2(r_s) + P_dg V(P_dg^T (r_s - t_s / theta)), t_s = A_s Binv_s r_s.  Hs: one shared hierarchy
    (the species are its columns) or one hierarchy per species."""

    def __init__(self, As, binvs, dg2cg, Hs, lmax, dtype=np.float64, mut=None):
        super().__init__(As, binvs, dg2cg, (Hs[0] if isinstance(Hs[0], list) else Hs)[0].n, dtype)
        self.shared = not isinstance(Hs[0], list)
        self.Hs, self.lmax, self.mut = Hs, lmax, mut

    def __call__(self, R, block_scale=None):
        """block_scale: (a mutation of the GMRES replica) the first pass over the cell blocks sees r_s times block_scale[s]"""
        cr, ctt, theta = _cheb2_coefficients(self.lmax, self.wd)
        Z, C = [], []
        for s, (A, Bi, r) in enumerate(zip(self.A, self.binv, R)):
            t = A @ _blocks(Bi, r if block_scale is None else block_scale[s] * r)
            Z.append(_blocks(Bi, cr * r - ctt * t))
            C.append(r - (1 / theta) * t)
        E = self.coarse(self.Hs, C, self.mut) if self.shared else [self.coarse(H, [c], self.mut)[0] for H, c in zip(self.Hs, C)]
        return [z + e for z, e in zip(Z, E)]


def bicgstab(As, bs, precond, iters, dtype=np.float64, x0=None):
    """`iters` iterations of bicgstab_impl from x0 (default 0) for the species' systems (their scalars are separate, the
    preconditioner sees all of them); the first iteration in the folded form p = r.  Returns [nsys, n]."""
    wd = np.float64 if dtype == "fsum" else dtype
    A = [_FsumCsr(M) if dtype == "fsum" else sp.csr_matrix(M).astype(wd) for M in As]
    ns = len(A)
    r = [np.asarray(b).astype(wd) for b in bs]                          # x0 = 0
    x = [np.zeros_like(b) for b in r]
    if x0 is not None:                                                  # k_bi_init: r = b - A x0
        x = [np.asarray(v).astype(wd).ravel().copy() for v in x0]
        r = [r[s] - A[s] @ x[s] for s in range(ns)]
    rhat = [v.copy() for v in r]
    rho = [b @ b for b in r]
    p = v = None
    alpha, omega, beta = [wd(1)] * ns, [wd(1)] * ns, [wd(0)] * ns
    for it in range(iters):
        p = [r[s].copy() if it == 0 else r[s] + beta[s] * (p[s] - omega[s] * v[s]) for s in range(ns)]
        y = precond(p)
        v = [A[s] @ y[s] for s in range(ns)]
        alpha = [rho[s] / (rhat[s] @ v[s]) for s in range(ns)]
        r = [r[s] - alpha[s] * v[s] for s in range(ns)]
        z = precond(r)
        t = [A[s] @ z[s] for s in range(ns)]
        omega = [(t[s] @ r[s]) / (t[s] @ t[s]) for s in range(ns)]
        x = [x[s] + alpha[s] * y[s] + omega[s] * z[s] for s in range(ns)]
        r = [r[s] - omega[s] * t[s] for s in range(ns)]
        rho_new = [rhat[s] @ r[s] for s in range(ns)]
        beta = [(rho_new[s] / rho[s]) * (alpha[s] / omega[s]) for s in range(ns)]
        rho = rho_new
    return np.stack(x)


# ---- restarted GMRES (krylov.hip: gmres_impl, krylov_scalar.hpp: gm_scalar_op) -----------------------------------------------------------
GM_BATCH = 8                                                            # inner products per k_gm_dots pass
GM_MUTATIONS = ("dots_past_8", "partial_batch", "skip_rotation", "no_normalise", "update_from_V", "short_backsub", "swap_y",
                "stale_restart")
_RUNNING, _CONVERGED, _CYCLE_DONE = 0, 1, 4                             # KrylovStatus


class _GmSystem:
    """one species: its iterate, basis, Hessenberg columns, rotations and scalars"""

    def __init__(self, wd, x0):
        self.wd, self.x = wd, x0
        self.flag, self.iter, self.cycles, self.margin = _RUNNING, 0, [], math.inf
        self.res = self.tol = self.t2 = self.beta = None

    def new_cycle(self, r, rr):
        wd = self.wd
        self.beta = np.sqrt(rr)
        self.V, self.Z, self.H = [r * (1 / self.beta)], [], []          # (k_gm_scale_binv: times the reciprocal, KS_ALPHA)
        self.cs, self.sn, self.g = [], [], [self.beta]
        self.k = 0
        need = self.tol / self.res if self.res > 0 else wd(1)
        self.t2 = self.beta * min(wd(0.5) * need, wd(0.1))

    def decide(self, value, threshold):
        """value <= threshold, and how far from flipping (relative to the threshold)"""
        if threshold > 0:
            self.margin = min(self.margin, float(abs(value - threshold) / threshold))
        return value <= threshold

    def y(self, mut=None):
        """OP_GM_SOLVE: back substitution over the cycle's k columns"""
        k = self.k - 1 if mut == "short_backsub" else self.k
        y = [self.wd(0)] * self.k
        for i in range(k - 1, -1, -1):
            t = self.g[i]
            for l in range(i + 1, k):
                t = t - self.H[l][i] * y[l]
            y[i] = t / self.H[i][i] if self.H[i][i] != 0 else self.wd(0)
        return y


def _gm_update(S, ys, mut):
    """k_gm_lincomb: x + sum_i y_i Z_i of every species that is running or has its cycle done"""
    out = []
    for s, (st, y) in enumerate(zip(S, ys)):
        x = st.x
        if st.flag in (_RUNNING, _CYCLE_DONE):
            for yi, zi, vi in zip(y, st.Z, st.V):
                x = x + yi * (vi if mut == "update_from_V" else zi)
        out.append(x)
    return out


def gmres_run(As, bs, precond, maxit, restart, dtype, mut=None, x0=None, tols=None, min_it=0, norm=None, reverse=False, snapshots=()):
    """The lockstep loop of gmres_impl with a look after every column (check_every = 1; what the host sees does not change the
    result: tests/test_gpu_krylov.py).  tols: per species the tolerance of the test on the true residual in `norm` (None: one that
    cannot be reached -- every cycle then has `restart` columns).  reverse: inner products and norms summed from the other end.
    Returns (the species' _GmSystem, {k: iterates had the solve ended with maxit = k} for k in snapshots)."""
    wd = np.float64 if dtype == "fsum" else dtype
    A = [_FsumCsr(M) if dtype == "fsum" else sp.csr_matrix(M).astype(wd) for M in As]
    ns, m = len(A), int(restart)
    b = [np.asarray(v).astype(wd) for v in bs]
    assert 2 <= m <= 30 and mut in (None,) + GM_MUTATIONS

    def dot(u, v):
        return np.dot(u[::-1].copy(), v[::-1].copy()) if reverse else np.dot(u, v)

    free = tols is not None
    S = [_GmSystem(wd, np.zeros_like(b[s]) if x0 is None else np.asarray(x0[s]).astype(wd)) for s in range(ns)]

    def residual(first, stale=None):                                    # residual(): k_bi_init behind the operator, OP_GM_INIT / OP_GM_RESTART
        for s, st in enumerate(S):
            if st.flag == _CONVERGED:
                continue
            r = b[s] - A[s] @ (st.x if stale is None else stale[s])
            rr = dot(r, r)
            if free:
                st.res = wd(norm(r))
                if first:
                    st.tol = wd(tols[s])
            else:
                st.res, st.tol = np.sqrt(rr), wd(0)
            if rr == 0 or (free and st.iter >= min_it and st.decide(st.res, st.tol)):
                st.flag = _CONVERGED
                continue
            st.flag = _RUNNING
            st.new_cycle(r, rr)

    residual(True)
    snap, it = {}, 0
    if 0 in snapshots:
        snap[0] = np.stack([st.x for st in S])
    while any(st.flag != _CONVERGED for st in S) and it < maxit:
        j = 0
        while j < m and any(st.flag == _RUNNING for st in S) and it < maxit:
            run = [s for s in range(ns) if S[s].flag == _RUNNING]
            # an idle species' column of the shared preconditioner call carries nothing the others read (the columns are independent)
            Vj = [S[s].V[j] if s in run else np.zeros_like(b[s]) for s in range(ns)]
            if mut == "no_normalise":                                   # k_gm_scale_binv: y = Binv v before v *= 1 / h_{j,j-1} (1 / beta)
                Zj = precond(Vj, block_scale=[(S[s].beta if j == 0 else S[s].hn) if s in run else wd(1) for s in range(ns)])
            else:
                Zj = precond(Vj)
            for s in run:
                st = S[s]
                st.Z.append(Zj[s])
                w = A[s] @ Zj[s]
                h = [dot(w, st.V[i]) for i in range(j + 1)]             # k_gm_dots: all from the unmodified w
                if mut == "dots_past_8":
                    h[GM_BATCH:] = [wd(0)] * len(h[GM_BATCH:])
                if mut == "partial_batch" and (j + 1) % GM_BATCH:
                    lo = (j + 1) // GM_BATCH * GM_BATCH
                    h[lo:] = [wd(0)] * (j + 1 - lo)
                for i in range(j + 1):                                  # k_gm_update
                    w = w - h[i] * st.V[i]
                hn = np.sqrt(dot(w, w))
                h.append(hn)                                            # OP_GM_NORM
                for i in range(j):
                    if mut == "skip_rotation" and i == 0:
                        continue
                    t = st.cs[i] * h[i] + st.sn[i] * h[i + 1]
                    h[i + 1] = -st.sn[i] * h[i] + st.cs[i] * h[i + 1]
                    h[i] = t
                den = np.sqrt(h[j] * h[j] + hn * hn)
                st.cs.append(h[j] / den if den > 0 else wd(1))
                st.sn.append(hn / den if den > 0 else wd(0))
                h[j] = den
                st.g.append(-st.sn[j] * st.g[j])
                st.g[j] = st.cs[j] * st.g[j]
                st.H.append(h)
                st.hn = hn
                st.V.append(w * ((1 / hn) if hn > 0 else wd(0)))        # (KS_OMEGA)
                st.k = j + 1
                st.iter += 1
                est = abs(st.g[j + 1])
                early = st.iter >= min_it and (hn == 0 or (free and j + 1 < m and st.decide(est, st.t2)))
                if early or j + 1 >= m:
                    st.flag = _CYCLE_DONE
            j += 1
            it += 1
            if it in snapshots and it < maxit:
                ys = [st.y(mut) if st.flag in (_RUNNING, _CYCLE_DONE) else None for st in S]
                snap[it] = np.stack(_gm_update(S, ys, None if mut == "swap_y" else mut))
        ys = [st.y(mut) if st.flag in (_RUNNING, _CYCLE_DONE) else None for st in S]
        if mut == "swap_y" and ys[0] is not None and ys[1] is not None:
            assert len(ys[0]) == len(ys[1])
            ys[0], ys[1] = ys[1], ys[0]
        old = [st.x for st in S]
        for st, x in zip(S, _gm_update(S, ys, mut)):
            if st.flag in (_RUNNING, _CYCLE_DONE):
                st.cycles.append(st.k)
                st.Z_done = st.Z                                        # (kept for the CPU tests: the next cycle starts a new list)
            st.x = x
        residual(False, old if mut == "stale_restart" else None)
    if maxit in snapshots:
        snap[maxit] = np.stack([st.x for st in S])
    return S, snap


def gmres(As, bs, precond, iters, restart=30, dtype=np.float64, mut=None, x0=None, reverse=False):
    """x after `iters` columns of gmres_impl from x0 (default 0) at a tolerance that cannot be reached: right preconditioning with the
    Z_j = M^-1 V_j kept, one classical Gram-Schmidt pass, the Givens rotations of gm_scalar_op, back substitution over the columns of
    the (possibly unfinished) cycle, x += sum y_i Z_i, restart from the true residual after `restart` columns.  The species' scalars
    are separate, the preconditioner sees all of them.  iters: a count -> [nsys, n]; a sequence of counts -> {count: [nsys, n]} from
    one run (the iterate after k columns is what a solve with maxit = k returns: the update of the unfinished cycle is applied).
    mut: one of GM_MUTATIONS; the snapshots of a run apply all of them but swap_y and stale_restart (the last count has those too)."""
    ks = (iters,) if np.isscalar(iters) else tuple(iters)
    _, snap = gmres_run(As, bs, precond, max(ks), restart, dtype, mut=mut, x0=x0, reverse=reverse, snapshots=ks)
    return snap[iters] if np.isscalar(iters) else snap


def gmres_free(As, bs, precond, tols, norm, restart=30, dtype=np.float64, min_it=0, maxit=1000, reverse=False):
    """the solve as the device runs it to convergence: T2 = beta min(0.5 tol / res, 0.1); a species' cycle ends at the first column
    whose estimate is <= T2 (iteration count >= min_it) or at column `restart`; it then idles until every species' cycle is done, all
    update and restart together, and the true residual in `norm` against tols[s] decides.  Per species a dict: x, niter, cycles (the
    column count of every cycle), margin (the smallest relative distance of a decision from its threshold), res (the last norm)."""
    S, _ = gmres_run(As, bs, precond, maxit, restart, dtype, tols=tols, min_it=min_it, norm=norm, reverse=reverse)
    assert all(st.flag == _CONVERGED for st in S), "the replica did not converge"
    return [dict(x=st.x, niter=st.iter, cycles=tuple(st.cycles), margin=st.margin, res=float(st.res)) for st in S]


# ---- which kernel instantiations a hierarchy reaches -----------------------------------------------------------------------------------
def launches(levels, ncol):
    """set of (kernel, G, NC) that restrict_tail and amg_vcycle_eager launch through by_density"""
    nc = 2 if ncol % 2 == 0 else 1
    out = set()

    def hit(kernel, M):
        out.add((kernel, band_G(sp.csr_matrix(M)), nc))
    nl = len(levels)
    if nl > 1 and levels[0].cheb_degree == 0:                           # amg_restrict.hip: restrict_tail
        hit("k_csr<0>", levels[0].R)
    for l in range(nl - 1):                                             # the way down
        L = levels[l]
        if L.cheb_degree == 0:
            if l > 0:
                hit("k_csr<0>", L.R)
            continue
        if L.cheb_degree > 1:
            hit("k_cheb_step", L.A)
        hit("k_csr<1>", L.A)
        hit("k_csr_first" if l + 1 < nl - 1 and levels[l + 1].cheb_degree > 0 else "k_csr<0>", L.R)
    for l in range(nl - 2, -1, -1):                                     # and up
        L = levels[l]
        if L.cheb_degree == 0:
            hit("k_csr<0>", L.P)
            continue
        hit("k_csr<2>", L.P)
        hit("k_cheb_first_res", L.A)
    return out


# ---- hand-built hierarchies ------------------------------------------------------------------------------------------------------------
def _pattern(rng, nrows, ncols, lengths):
    rows = np.repeat(np.arange(nrows), lengths)
    cols = np.concatenate([rng.choice(ncols, size=k, replace=False) for k in lengths]) if nrows else np.zeros(0, int)
    return rows, cols


def _lengths(rng, nrows, ncols, avg):
    """row lengths around `avg`; where they fit, lengths 1 modulo U * G of both unrollings sit in the first rows (5, 17, 33, 257)"""
    ln = np.clip(rng.poisson(avg, size=nrows), 1, ncols)
    special = [k for k in (5, 17, 33, 257) if k <= ncols and 0.4 * avg <= k <= 2.7 * avg]
    ln[:len(special)] = special[:nrows]
    return ln


def _spd(rng, n, avg, scale):
    """sparse, symmetric, strictly diagonally dominant; about `avg` entries per row"""
    half = max((avg - 1.0) / 2.0, 0.0)
    r, c = _pattern(rng, n, n, np.clip(rng.poisson(half, size=n), 0, n))
    keep = r != c
    S = sp.coo_matrix((-rng.uniform(0.1, 1.0, size=int(keep.sum())), (r[keep], c[keep])), shape=(n, n)).tocsr()
    S = S + S.T
    off = np.asarray(abs(S).sum(axis=1)).ravel()
    A = (S + sp.diags(off * rng.uniform(1.002, 1.05, size=n) + 0.01)).tocsr() * (scale / (off.mean() + 0.01))   # mean diagonal ~ scale
    A.sort_indices()
    # every value 2.5e-8 (less than half an fp32 step) above an fp32 number: the device's rounding is then a shift of the whole matrix
    # in one direction, which a replica that forgets it cannot hide in averaging sums
    A.data = A.data.astype(np.float32).astype(np.float64) * (1.0 + 2.5e-8)
    return A


def _prolongator(rng, n, ncoarse, avg):
    ln = _lengths(rng, n, ncoarse, avg)
    r, c = _pattern(rng, n, ncoarse, ln)
    if ncoarse - 1 not in c:
        c[0] = ncoarse - 1                                              # every coarse dof down to the last one has a say
    P = sp.coo_matrix((rng.uniform(1.0, 3.0, size=len(r)) / np.repeat(ln, ln), (r, c)), shape=(n, ncoarse)).tocsr()
    P.sort_indices()
    return P


def synthetic(sizes, dens_A, dens_P, degrees, scale, seed):
    """Levels of sizes `sizes` with about dens_A[l] / dens_P[l] entries per row of A_l / P_l (R_l = P_l^T), Chebyshev degrees
    `degrees` and a dense symmetric positive fp32 matrix G G^T / n + I on the last one.  `scale`: size of the entries of A (the V-cycle
    then answers with about b / scale, like the cell blocks of the operator it is added to)."""
    rng = np.random.default_rng(seed)
    levels = []
    for l, n in enumerate(sizes):
        lv = _Level()
        last = l == len(sizes) - 1
        lv.A = _spd(rng, n, 3.0 if last else dens_A[l], scale)
        lv.dinv = 1.0 / lv.A.diagonal()
        # (the spectrum of D^-1 A lies in (0, 2), most of it near 1: a generous rho leaves every level about half of its residual, so
        # that all levels have their share in the result)
        lv.rho = float(rng.uniform(2.6, 3.4))
        lv.cheb_lower = float(rng.uniform(0.1, 0.3))
        lv.cheb_degree = 0 if last else int(degrees[l])
        if not last:
            lv.P = _prolongator(rng, n, sizes[l + 1], dens_P[l])
            lv.R = lv.P.T.tocsr()
            lv.R.sort_indices()
        levels.append(lv)
    n = sizes[-1]
    G = rng.standard_normal((n, n))
    levels[-1].pinv = ((G @ G.T / n + np.eye(n)) / scale).astype(np.float32)
    return levels


COARSE_N = (1, 2, 33, 255, 257, 769, 1030, 2051)
# the hierarchies of synthetic_set: the CPU coverage assertion and the device tests (one column: EMI, two: KNP) run this same list
SYNTHETIC = ("bands", "bands_t0", "mid") + tuple("coarse_%d" % n for n in COARSE_N)


def drop_tail_targets(levels, ncol):
    """(level, matrix) pairs the V-cycle uses that have a row of length 1 modulo U * G of the variant the matrix selects"""
    out = []
    for l, lv in enumerate(levels[:-1]):
        for key in ("A", "P", "R"):
            if key == "A" and lv.cheb_degree == 0:
                continue
            if _drop_tail(sp.csr_matrix(getattr(lv, key)), ncol)[1]:
                out.append((l, key))
    return out


def synthetic_set(n0, scale):
    """name -> levels: the hierarchies to run on the device, for a conforming space of n0 dofs"""
    out = {
        # every density band among the A's, P's and R's; all smoother degrees
        "bands": synthetic((n0, 300, 150, 70, 33), (25, 120, 60, 8), (105, 8, 5, 20), (2, 3, 1, 2), scale, 11),
        # the same with a transfer-only finest level, as the EMI production hierarchy had it
        "bands_t0": synthetic((n0, 300, 150, 70, 33), (25, 120, 60, 8), (105, 8, 5, 20), (0, 2, 3, 1), scale, 11),
        # a restriction in the top band that also carries the next level's first smoother update (k_csr_first<64, .>)
        "mid": synthetic((n0, 140, 40), (50, 100), (60, 30), (1, 2), scale, 12),
    }
    dens = {1: (6, 1), 2: (30, 1), 33: (70, 4), 255: (110, 5), 257: (10, 60), 769: (45, 120), 1030: (20, 20), 2051: (8, 3)}
    for k, n in enumerate(COARSE_N):
        out["coarse_%d" % n] = synthetic((n0, n), (dens[n][0],), (dens[n][1],), (1 + k % 3,), scale, 20 + k)
    return out


# ---- the k-iteration observable on the oracle's matrices ------------------------------------------------------------------------------
EXTRA_IONS = dict(X=(1.0, 1.6e-9), Y=(-1.0, 1.8e-9))                    # (z, D) of the ions beyond K, Cl, Na (monovalent: see
                                                                        # test_knp_solve_with_other_species_counts)


def four_materials(pb):
    """[D per ion] with four D tuples over the cells: D of every ion times 0.5 in the intracellular cells (tag 1) and times 1.5 in the
    extracellular cells whose centroid lies in the upper half of x; the second ion times 0.8 more in that upper half, inside and outside: four D tuples, and interior SIPG facets
    (tag 0) between different ones (the x mid-plane cuts both subdomains).  (Which ion and which factor is the reference's choice:
    with the first ion times 1.25 instead, BiCGStab on the P2 box comes close to a breakdown in its second iteration -- the float64
    and extended-precision replicas of x_2 differ by 6e-9 of x_2, the bound would be 1.9e-7 -- so that case compares nothing.)"""
    m = pb.mesh
    x = m.coords[m.cells].mean(axis=1)[:, 0]
    upper = x > 0.5 * (m.coords[:, 0].min() + m.coords[:, 0].max())
    f = np.where(pb.cell_tags == 1, 0.5, np.where(upper, 1.5, 1.0))
    return [ion["D"] * f * (np.where(upper, 0.8, 1.0) if i == 1 else 1.0) for i, ion in enumerate(pb.ions)]


class Host:
    """One of the test meshes ("box_P1": small_3d((8, 4, 4)), "box_P2": small_3d((6, 3, 3)) with DG-P2, "2D_P1": make_mesh_2D(0)) with
    the oracle's problem in the seeded synthetic state, its matrices (krylov_ref.Ref) and the conforming map of the preconditioner.
    names: ions of the problem, the last one eliminated (default: the K / Cl / Na problem of the examples).
    phi_scale: factor on the synthetic potential (1: cell Peclet number 5.4, the per-cell blocks; 0.05: 0.270 and 0.01: 0.054, the
    drift-free class table of solve.hip).  materials: four D tuples instead of one (`four_materials`)."""

    def __init__(self, mesh, names=None, phi_scale=1.0, materials=False):
        import knpemi_oracle as ko
        import krylov_ref as kr
        from common import synthetic_state, small_3d
        from knpemidg import amg
        self.mesh_name, self.materials, p = mesh, bool(materials), (2 if mesh.endswith("P2") else 1)
        if mesh == "2D_P1":
            from knpemidg.mesh import make_mesh_2D
            self.mt = make_mesh_2D(0)
        else:
            self.mt = small_3d((8, 4, 4) if p == 1 else (6, 3, 3))
        m, s, f = self.mt
        if names is None:
            pb = ko.build_idealized(m, s.array(), f.array(), p=p, membrane_tags=(1,))
        else:
            P = ko.idealized_params()
            z = dict(P["z"], **{n: v[0] for n, v in EXTRA_IONS.items()})
            D = dict(P["D"], **{n: v[1] for n, v in EXTRA_IONS.items()})
            ions = [dict(name=n, z=z[n], D=np.full(m.num_cells(), D[n])) for n in names]
            pb = ko.Problem(m, s.array().astype(np.int64), f.array(), p, ions, P, membrane_tags=(1,))
            rng = np.random.default_rng(7)
            pb.c = rng.uniform(80.0, 120.0, size=pb.c.shape)
            pb.c_prev_n = pb.c * (1 + 1e-3 * rng.uniform(-1, 1, size=pb.c.shape))
            pb.c_elim = rng.uniform(80.0, 120.0, size=pb.c_elim.shape)
        synthetic_state(pb)
        pb.phi = phi_scale * pb.phi
        if materials:
            for ion, D in zip(pb.ions, four_materials(pb)):
                ion["D"] = D
        self.pb, self.ref, self.nd = pb, kr.Ref(pb), pb.nd                # (after the changes above: its matrices see them)
        self.cs = amg.ConformingSpace(m, f.array(), (1,))
        self.cs2 = amg.ConformingSpaceP2(self.cs) if p != 1 else None
        self.dg2cg = np.asarray((self.cs2 or self.cs).dof)
        self.ncg = int(self.dg2cg.max()) + 1
        self._knp = self._tab = None

    def variant(self, phi=None, dt=None, D=None, c=None):
        """this host with another potential [nc, nd], time step or diffusion coefficients [ions, nc]: the KNP matrices and both block
        sets follow (assembled at first use), the mesh, the state and the EMI side (`ref`) are shared.  For potentials and
        coefficients that change on a live device.  c = (solved concentrations [N_ions, nc, nd], eliminated one [nc, nd]): kappa, and
        with it A_emi, b_emi and binv_emi of `ref`, follow (assembled here; the KNP matrices do not depend on c, their loads do)."""
        import copy
        h = copy.copy(self)
        h.pb = copy.copy(self.pb)
        h._knp = None
        if phi is not None:
            h.pb.phi = np.array(phi, dtype=np.float64).reshape(self.pb.phi.shape)
        if dt is not None:
            h.pb.dt, h._tab = float(dt), None
        if D is not None:
            h.pb.ions = [dict(ion, D=np.array(d, dtype=np.float64)) for ion, d in zip(self.pb.ions, D)]
            h._tab = None
        if c is not None:
            import krylov_ref as kr
            h.pb.c = np.array(c[0], dtype=np.float64).reshape(self.pb.c.shape)
            h.pb.c_elim = np.array(c[1], dtype=np.float64).reshape(self.pb.c_elim.shape)
            h.ref = kr.Ref(h.pb)
            return h
        h.ref = copy.copy(self.ref)
        h.ref.pb = h.pb
        return h

    def emi_levels(self, level0_degree=None):
        """the production hierarchy (Case.upload_amg of test_gpu_krylov.py); level0_degree: Chebyshev degree of a P1 mesh's finest
        conforming level (KNP_AMG_DEGREE0_EMI for this build; None: as the environment has it)"""
        import os
        from knpemidg import amg
        tags = self.mt[2].array()
        mem = sorted({int(t) for t in np.unique(tags[self.pb.mem])})
        keep = os.environ.get("KNP_AMG_DEGREE0_EMI")
        if level0_degree is not None:
            os.environ["KNP_AMG_DEGREE0_EMI"] = str(int(level0_degree))
        try:
            return amg.build_emi_levels(self.cs, self.cs2, tags, mem, self.pb.kappa(), self.pb.C_phi)
        finally:
            if level0_degree is not None:
                os.environ.pop("KNP_AMG_DEGREE0_EMI")
                if keep is not None:
                    os.environ["KNP_AMG_DEGREE0_EMI"] = keep

    def local_problem(self, loc):
        """the oracle's problem of one rank (knpemidg.partition.LocalMesh: owned cells, then ghosts) with coefficients and state
        sliced from the global arrays -- what a partitioned run holds behind a halo exchange"""
        import knpemi_oracle as ko
        pbg, cg = self.pb, loc.cells_global
        sub_l, surf_l = loc.localize(self.mt[1], self.mt[2], pbg.membrane_tags)
        ions = [dict(ion, D=np.asarray(ion["D"])[cg].copy()) for ion in pbg.ions]
        pbl = ko.Problem(loc.mesh, sub_l.array().astype(np.int64), surf_l.array(), pbg.p, ions, ko.idealized_params(),
                         membrane_tags=pbg.membrane_tags)
        assert (pbl.dt, pbl.C_phi, pbl.tau, pbl.splitting) == (pbg.dt, pbg.C_phi, pbg.tau, pbg.splitting)
        pbl.c, pbl.c_prev_n, pbl.c_elim, pbl.phi = pbg.c[:, cg].copy(), pbg.c_prev_n[:, cg].copy(), pbg.c_elim[cg].copy(), pbg.phi[cg].copy()
        pbl.phi_M = pbg.phi_M[loc.facets_global].copy()
        for name in pbg.I_ch:
            pbl.I_ch[name] = pbg.I_ch[name][loc.facets_global].copy()
        return pbl

    def knp_groups(self, level0_degree=1):
        """[(members, levels)]: the production hierarchies of the solved species (amg.build_knp_groups, as knpemidg/solver.py calls
        it; every ion of the host has one diffusion coefficient on all cells)"""
        from knpemidg import amg
        tags = np.asarray(self.mt[1].array())
        D_subs = [{int(t): float(ion["D"][0]) for t in np.unique(tags)} for ion in self.pb.ions[:self.pb.N_ions]]
        assert not self.materials and all(np.all(ion["D"] == ion["D"][0]) for ion in self.pb.ions)
        return amg.build_knp_groups(self.cs, self.cs2, tags, D_subs, self.pb.dt, level0_degree)

    def scale(self, knp=False):
        """entry size of a synthetic hierarchy whose V-cycle answers in the size of the cell blocks' part of the preconditioner"""
        A = self.knp()[0][0] if knp else self.ref.A_emi
        return float(A.diagonal().mean()) * self.pb.ndof / self.ncg

    def knp(self):
        """([A_k], [fp32 cell-block inverses of A_k], [oracle b_k]) of the solved species"""
        if self._knp is None:
            import krylov_ref as kr
            mats = [self.ref.knp(k) for k in range(self.pb.N_ions)]
            self._knp = ([A for A, _ in mats], [kr.block_inverses(A, self.nd) for A, _ in mats], [b.ravel() for _, b in mats])
        return self._knp

    def knp_table_blocks(self):
        """[fp32 cell-block inverses of A_k assembled at phi = 0]: what build_bj_table (solve.hip) gathers its table from -- one launch of
        the per-cell kernel with a zero drift coefficient, then the representatives' blocks (k_bj_gather).  Listed per cell here; that
        the cells of one table key hold the same bits is asserted by tests/test_amg_ref_host.py (`table_keys`)."""
        if self._tab is None:
            import krylov_ref as kr
            import knpemi_oracle as ko
            keep = self.pb.phi
            self.pb.phi = np.zeros_like(keep)
            try:
                self._tab = [kr.block_inverses(ko.assemble_knp(self.pb, k).tocsr(), self.nd) for k in range(self.pb.N_ions)]
            finally:
                self.pb.phi = keep
        return self._tab

    def blocks(self, which):
        """"cell": the per-cell inverses with the drift of the host's potential; "table": the drift-free ones; a list: itself"""
        if isinstance(which, str):
            return {"cell": lambda: self.knp()[1], "table": self.knp_table_blocks}[which]()
        return list(which)

    def table_keys(self):
        """per cell, the key of build_bj_table: (geometry class, material id of the D tuple over all ions, kind of each of the four
        facets: 0 interior SIPG, 1 membrane, 2 exterior, 3 interior and inactive -- FK_* of knpemi_internal.hpp)"""
        from knpemidg import _abi
        m, pb = self.mt[0], self.pb
        nc = m.num_cells()
        cls = _abi.geometry_classes(m, np.arange(nc))
        assert cls is not None, "not a structured 3D mesh"
        D = np.stack([ion["D"] for ion in pb.ions], axis=1)
        mat = np.unique(D, axis=0, return_inverse=True)[1].ravel()
        cf = np.asarray(m.cell_facets)
        interior = np.asarray(m.facet_cells)[cf, 1] >= 0
        tags = pb.facet_tags[cf]
        kind = np.where(~interior, 2, np.where(tags == 0, 0, np.where(np.isin(tags, pb.membrane_tags), 1, 3)))
        return [(int(cls[0][c]), int(mat[c])) + tuple(int(v) for v in kind[c]) for c in range(nc)]

    def cell_peclet(self):
        zmax = max(abs(ion["z"]) for ion in self.pb.ions[:-1])
        return self.pb.psi * zmax * (self.pb.phi.max(axis=1) - self.pb.phi.min(axis=1))

    def peclet(self):
        """solve.hip: k_cell_peclet -- above 0.5 the KNP solve uses the per-cell block inverses (drift included), as `knp` does; up to
        0.5 the drift-free class table (`knp_table_blocks`)"""
        return float(self.cell_peclet().max())


def emi_xk(host, levels, cheb, k, dtype=np.float64, b=None, mut=None, dist=None, x0=None, binv=None, lmax=None):
    """x_k of the device's EMI PCG from x_0 (default 0) with the two-level preconditioner over `levels`; cheb: the Chebyshev DG smoother;
    dist: a `Dist0` -- level 0 of the V-cycle in the row-distributed form of that partition (or the pair `store` takes).
    binv: other cell blocks than those of the host's matrix (lagged ones); lmax: the spectral bound itself, where the device keeps one
    (default: estimated on these matrices and blocks from b).  levels = None: the cell blocks alone (a context without a hierarchy)."""
    import types
    import krylov_ref as kr
    ref = host.ref
    b = ref.b_emi if b is None else np.asarray(b, dtype=np.float64).ravel()
    binv = ref.binv_emi if binv is None else np.asarray(binv, dtype=np.float64)
    sysm = types.SimpleNamespace(A_emi=ref.A_emi, b_emi=b, binv_emi=binv)
    if levels is None:
        return kr.pcg(sysm, 0.0, 0.0, x0=x0, iters=k, dtype=dtype)[0]
    if lmax is None:
        lmax = bj_lambda_max([ref.A_emi], [binv], [b]) if cheb else 0.0
    H = store(levels, dtype, mut, dist=dist)
    M = EmiPrecond(ref.A_emi, binv, host.dg2cg, H, lmax, dtype, mut)
    return kr.pcg(sysm, 0.0, 0.0, x0=x0, precond=M, iters=k, dtype=dtype)[0]


def knp_lmax(host, blocks, bs):
    """the spectral bound a KNP solve on `host`'s matrices estimates from the right-hand sides bs with the block set `blocks`"""
    return bj_lambda_max(host.knp()[0], host.blocks(blocks), [np.asarray(b, dtype=np.float64).ravel() for b in bs])


def _knp_system(host, levels, dtype, bs, lmax_bs, mut, blocks, lmax, dist=None):
    """(A_s, b_s, the two-level preconditioner) of a KNP solve on `host`'s matrices: the arguments of knp_xk"""
    As, _, b0 = host.knp()
    binvs = host.blocks(blocks)
    bs = b0 if bs is None else [np.asarray(b, dtype=np.float64).ravel() for b in bs]
    ns = len(As)
    if lmax is None:
        lmax = bj_lambda_max(As, binvs, bs if lmax_bs is None else lmax_bs)
    shared = hasattr(levels[0], "A")
    amg_mut = mut if isinstance(mut, tuple) else None       # (a name alone: one of GM_MUTATIONS)
    Hs = store(levels, dtype, amg_mut, ncol=ns, dist=dist) if shared else [store(lv, dtype, amg_mut, dist=dist) for lv in levels]
    return As, bs, KnpPrecond(As, binvs, host.dg2cg, Hs, lmax, dtype, amg_mut)


def knp_xk(host, levels, k, dtype=np.float64, bs=None, lmax_bs=None, mut=None, blocks="cell", lmax=None, method="bicgstab",
           reverse=False, dist=None, x0=None):
    """x_k [nsys, ndof] of the device's KNP solve from x_0 = 0 (x0 [nsys, ndof]: from there).  levels: one hierarchy shared by the species (its columns), or a
    list with one hierarchy per species.  lmax_bs: the right-hand sides the spectral bound was estimated from (default: bs).
    blocks: the cell blocks of the preconditioner and of the spectral bound -- "cell" (per-cell inverses with the drift), "table" (the
    drift-free class table of solve.hip) or an explicit list (lagged inverses of another potential: `Host.variant(...).blocks`).
    lmax: the spectral bound itself, where the device keeps one estimated on other matrices (`knp_lmax`).
    method: "bicgstab", or ("gmres", m) for GMRES restarted after m columns -- k may then be a sequence of counts (`gmres`), mut one
    of GM_MUTATIONS, and reverse sums the inner products from the other end.
    dist: a `Dist0` -- level 0 of the V-cycle in the row-distributed form of that partition."""
    As, bs, M = _knp_system(host, levels, dtype, bs, lmax_bs, mut, blocks, lmax, dist)
    if method == "bicgstab":
        return bicgstab(As, bs, M, k, dtype, x0=x0)
    assert method[0] == "gmres"
    return gmres(As, bs, M, k, method[1], dtype, mut=mut if isinstance(mut, str) else None, x0=x0, reverse=reverse)


def knp_gmres_free(host, levels, rtol, m, dtype=np.float64, bs=None, blocks="table", min_it=0, reverse=False):
    """the converged GMRES(m) solve of knp_knp_solve from x_0 = 0 at `rtol`: the stopping test is on the order-8 norm of the residual's
    density against KNP_D8_FACTOR rtol times that of the load (solve.hip).  Returns `gmres_free`'s list."""
    import krylov_ref as kr
    As, bs, M = _knp_system(host, levels, dtype, bs, None, None, blocks, None)
    tols = [kr.KNP_D8_FACTOR * rtol * host.ref.norm_d8(b) for b in bs]
    return gmres_free(As, bs, M, tols, host.ref.norm_d8, m, dtype, min_it=min_it, reverse=reverse)


# the GMRES cases the device runs (tests/test_gpu_amg.py): (mesh, solved species, hierarchy or one per species, block set, restart
# length m, the iteration counts k) -- "cell" at the synthetic potential, "table" at TABLE_PHI_SCALE times it.  With m = 30 the counts
# 9 / 10, 17 and 25 end in the second, third and fourth pass of k_gm_dots with 1 / 2, 1 and 1 inner products in it (cnt < 8), 30 is
# the full cycle (four passes, six in the last one) and 33 the first restart; m = 3 and m = 8 restart once and twice, the second
# time in an unfinished cycle.  tests/test_amg_ref_host.py asserts that every case has its bound and what the counts reach.
GM_KS = (1, 2, 9, 10, 17, 25, 30, 33)
GM_CASES = (("box_P1", 2, "coarse_257", "cell", 30, GM_KS),
            ("box_P1", 2, "coarse_257", "table", 30, GM_KS), ("box_P1", 2, "mid", "table", 30, GM_KS),
            ("box_P1", 2, "coarse_257", "table", 3, (5, 7)), ("box_P1", 2, "mid", "table", 3, (5, 7)),
            ("box_P1", 2, "coarse_257", "table", 8, (20,)), ("box_P1", 2, "mid", "table", 8, (20,)),
            ("box_P1", 3, "coarse_257", "cell", 30, (2, 10, 33)), ("box_P1", 3, "mid", "table", 30, (2, 10, 33)),
            ("box_P1", 2, ("coarse_257", "mid"), "cell", 30, (2, 10, 33)), ("box_P1", 2, ("coarse_257", "mid"), "table", 30, (2, 10, 33)),
            ("box_P2", 2, "coarse_769", "cell", 30, (3, 10)), ("box_P2", 2, "coarse_257", "table", 30, (3, 10)),
            ("2D_P1", 2, "mid", "cell", 30, (3, 10)), ("2D_P1", 2, "bands", "cell", 30, (3, 10)))
# converged solves on box_P1, two species, the class table: (hierarchy, rtol, m).  rtol 0.01 / 0.0025 / 0.001 put the test on the
# order-8 density norm at 0.2 / 0.05 / 0.02 of the load's
GM_FREE_CASES = (("coarse_257", 0.01, 30), ("mid", 0.01, 30), ("coarse_257", 0.0025, 8), ("mid", 0.0025, 8), ("coarse_257", 0.001, 30),
                 ("mid", 0.001, 30))


def gm_host_args(case):
    """the arguments of `Host` for one of GM_CASES"""
    mesh, ns, _, blocks = case[:4]
    return mesh, IONS[ns], (1.0 if blocks == "cell" else TABLE_PHI_SCALE), False


def gm_levels(sets, names):
    return sets[names] if isinstance(names, str) else [sets[n] for n in names]


def gm_columns(k, m):
    """the columns (within their cycles) that k iterations of GMRES(m) run"""
    return [it % m for it in range(k)]


def gm_batches(j):
    """(passes of k_gm_dots for column j, whether the last one is partial: cnt < 8)"""
    return -(-(j + 1) // GM_BATCH), (j + 1) % GM_BATCH != 0


def gm_reference(host, levels, blocks, m, ks, bs=None):
    """{k: (x64 [nsys, n], bounds [nsys], scales [nsys])}: the float64 replica of GMRES(m) after k iterations and the comparison bound
    per species -- `bound` over the float64 run, the float64 run with reversed sums and the extended-precision run"""
    ks = tuple(ks)
    run = lambda dtype, rev: knp_xk(host, levels, ks, dtype, bs=bs, blocks=blocks, method=("gmres", m), reverse=rev)
    x64, xrev, xhp = run(np.float64, False), run(np.float64, True), run(hp_dtype(), False)
    return {k: (x64[k], [bound(x64[k][s], xhp[k][s], xrev[k][s]) for s in range(len(x64[k]))],
                [float(np.abs(xhp[k][s]).max()) for s in range(len(x64[k]))]) for k in ks}


def gm_free_reference(host, levels, rtol, m, bs=None):
    """the converged solve three times (float64, float64 with reversed sums, extended precision): (the float64 run's list of
    `gmres_free`, bounds [nsys], scales [nsys], smallest decision margin of the three runs); the three runs must take the same
    decisions (iteration and cycle counts), else no comparison of iterates means anything"""
    r64 = knp_gmres_free(host, levels, rtol, m, bs=bs)
    rrev = knp_gmres_free(host, levels, rtol, m, bs=bs, reverse=True)
    rhp = knp_gmres_free(host, levels, rtol, m, hp_dtype(), bs=bs)
    for a, b, c in zip(r64, rrev, rhp):
        assert a["niter"] == b["niter"] == c["niter"] and a["cycles"] == b["cycles"] == c["cycles"], (a["cycles"], b["cycles"], c["cycles"])
    margin = min(r["margin"] for run in (r64, rrev, rhp) for r in run)
    return (r64, [bound(a["x"], c["x"], b["x"]) for a, b, c in zip(r64, rrev, rhp)], [float(np.abs(c["x"]).max()) for c in rhp], margin)


def at_peclet(host, pe):
    """`host` with its potential scaled to the cell Peclet number pe"""
    h = host.variant(phi=host.pb.phi * (pe / host.peclet()))
    assert abs(h.peclet() - pe) <= 1e-12
    return h


def one_cell_peclet(host, cell, pe=0.8, background=0.054):
    """`host` at the Peclet number `background`, but for `cell`, whose nodal potentials are stretched to `pe`"""
    low = at_peclet(host, background)
    phi = low.pb.phi.copy()
    phi[cell] *= pe / low.cell_peclet()[cell]
    h = host.variant(phi=phi)
    cp = h.cell_peclet()
    assert int(np.argmax(cp)) == cell and abs(cp[cell] - pe) <= 1e-12 and np.sort(cp)[-2] <= background + 1e-12
    return h


def switch_sequence(lo, bs):
    """The solves of a context whose potential changes ON THE DEVICE (no state upload, as in a time step) between `lo` (Peclet number
    0.27) and two higher ones (0.8, 0.7), x_0 = 0 likewise, by the rules of knp_knp_solve (solve.hip):

      * the Peclet number of a potential arrives with the status polls of the first solve at that potential: that solve still uses
        the block set of the previous potential, the next one the new set;
      * the table solves keep the age of the per-cell array at 0, so the first solve that falls back rebuilds it from the drift of the
        potential it runs at -- the array then holds the drift-free content the table build left there, or older inverses; later
        per-cell solves keep the array (KNP_BJ_LAG = 8): the one solve that still runs on it after the potential has returned applies
        the inverses of the OTHER potential;
      * the spectral bound (chebyshev_bound) is estimated from the right-hand side by the first solve, after a state upload and after
        a flip of the block set -- on the matrices and blocks of that solve; otherwise it is kept: no solve of the tests converges,
        so no reference iteration count exists (it_ref stays -1), and the age limit of 64 solves is not reached.

    Returns the steps: dict(tag, phi: the host whose potential goes to the device before the solve (or None), host: the matrices,
    blocks, lmax: the kept bound (None: estimated by this solve), wrong: {what a broken rule would give: (blocks, lmax)}).  The first
    step follows a state upload."""
    hi, hi2 = at_peclet(lo, 0.8), at_peclet(lo, 0.7)
    lm_lo = knp_lmax(lo, "table", bs)
    lm_hi = knp_lmax(hi, "cell", bs)
    T, C = "table", "cell"
    step = lambda tag, phi, host, blocks, lmax, **wrong: dict(tag=tag, phi=phi, host=host, blocks=blocks, lmax=lmax, wrong=wrong)
    return [
        step("1 low", lo, lo, T, None, per_cell=(C, None)),
        step("2 high, Peclet not seen yet", hi, hi, T, lm_lo, switched_at_once=(C, None), new_bound=(T, None)),
        step("3 high", None, hi, C, None, still_table=(T, lm_lo), bound_kept=(C, lm_lo), drift_free_array=(T, None)),
        step("4 low, Peclet not seen yet", lo, lo, hi.blocks(C), lm_hi, switched_at_once=(T, None), rebuilt=(C, lm_hi),
             new_bound=(hi.blocks(C), None)),
        step("5 low", None, lo, T, None, still_per_cell=(hi.blocks(C), lm_hi), bound_kept=(T, lm_hi)),
        step("6 low again", None, lo, T, lm_lo),
        step("7 high again, Peclet not seen yet", hi2, hi2, T, lm_lo, switched_at_once=(C, None), new_bound=(T, None)),
        step("8 high again", None, hi2, C, None, stale_array=(hi.blocks(C), None), bound_kept=(C, lm_lo)),
    ]


# ---- the partitioned comparison (tests/test_gpu_amg_partition.py, tests/amg_partition_worker.py) -------------------------------------------
# Production hierarchies with KNP_AMG_MAXCOARSE = 60 (both boxes then have a level below the finest one: [267, 52] on the P1 box,
# [679, 124, 26] on the P2 box).  A case: ("emi", level-0 degree, Chebyshev DG smoother, counts) or ("knp", solved species, block set,
# level-0 degree, None (BiCGStab) or the restart length of GMRES, counts); level-0 degree None: the P2 box (its top level has degree
# 2).  PART_GROUPS: (group, mesh, row-distributed level 0, {partition: cases}); one launch of the ranks serves a group's partition.
PART_MAXCOARSE = "60"
PART_GM_KS = (1, 2, 9, 10, 17, 20)                                     # with m = 8: the first and second restart behind 9 / 10 and 17,
                                                                        # 20 as in GM_CASES: a partial pass of k_gm_dots in every one
_EMI1 = (("emi", 1, False, (1, 2, 3)), ("emi", 1, True, (1, 2, 3)))
_KNP2 = (("knp", 2, "cell", 1, None, (1, 2)), ("knp", 2, "table", 1, None, (1, 2)))
# (x_2 and x_3 of the P2 box with the Chebyshev DG smoother are ill-conditioned: bounds 1.15e-9 and 1.53e-9 of the result)
_P2 = (("emi", None, False, (1, 2, 3)), ("emi", None, True, (1,)), ("knp", 2, "cell", None, None, (1, 2)))
PART_GROUPS = (
    ("P1-emi", "box_P1", True, {"slab2": _EMI1, "thin3": _EMI1,
                                "quad4": _EMI1 + tuple(("emi", d, cheb, (1, 2, 3)) for d in (0, 2) for cheb in (False, True))}),
    ("P1-knp2", "box_P1", True, {"slab2": _KNP2,
                                 "quad4": _KNP2 + (("knp", 2, "cell", 0, None, (1, 2)), ("knp", 2, "table", 1, 8, PART_GM_KS))}),
    ("P1-knp34", "box_P1", True, {"quad4": (("knp", 3, "cell", 1, None, (1, 2)), ("knp", 4, "table", 1, None, (1, 2)))}),
    ("P2", "box_P2", True, {"slab2": _P2, "quad4": _P2}),
    ("P1-replicated", "box_P1", False, {"slab2": _EMI1 + _KNP2[:1]}),
)
PART_LAUNCHES = tuple((g, p) for g, _, _, parts in PART_GROUPS for p in parts)


def part_group(name):
    return next(g for g in PART_GROUPS if g[0] == name)


def part_partition(mesh, name):
    """the partitions of the comparison: two x-slabs; three x-slabs whose middle one has no interior cell; the four quadrants of the
    y-z plane about the box centre (conforming dofs on the centre line have four owners, ranks 0 and 3 share dofs and no facet)"""
    from knpemidg.partition import Partition
    if name == "slab2":
        return Partition(mesh, 2, method="slab")
    if name == "thin3":
        return Partition(mesh, 3, method="slab", fractions=[0.0, 0.49, 0.51, 1.0])
    assert name == "quad4"
    mid = mesh.cell_midpoints()
    centre = 0.5 * (mesh.coords.min(axis=0) + mesh.coords.max(axis=0))
    return Partition(mesh, owner=(mid[:, 1] > centre[1]).astype(np.int32) + 2 * (mid[:, 2] > centre[2]).astype(np.int32))


def part_host_key(mesh, case):
    """the arguments of `Host` for a case (EMI cases run on the host of the two-species cases at the synthetic potential)"""
    if case[0] == "emi":
        return mesh, None, 1.0, False
    return mesh, IONS[case[1]], (1.0 if case[2] == "cell" else TABLE_PHI_SCALE), False


def part_case_id(case):
    if case[0] == "emi":
        return "emi deg0=%s cheb=%d" % (case[1], case[2])
    return "knp ns=%d %s deg0=%s %s" % (case[1], case[2], case[3], "bicgstab" if case[4] is None else "gmres(%d)" % case[4])


def part_levels(host, case):
    """the production hierarchy of a case (KNP: the one all species share), built under KNP_AMG_MAXCOARSE = PART_MAXCOARSE"""
    import os
    assert os.environ.get("KNP_AMG_MAXCOARSE") == PART_MAXCOARSE
    if case[0] == "emi":
        levels = host.emi_levels(case[1])
    else:
        groups = host.knp_groups(1 if case[3] is None else case[3])
        assert len(groups) == 1 and list(groups[0][0]) == list(range(case[1])), "the species do not share one hierarchy"
        levels = groups[0][1]
    assert len(levels) >= 2 and (case[0] == "emi" and case[1] is None or levels[0].cheb_degree == (case[1] if case[0] == "emi" else
                                                                                                 2 if case[3] is None else case[3]))
    return levels


def part_xk(host, levels, case, dtype=np.float64, dist=None, mut=None, reverse=False, bs=None, ks=None):
    """{k: x_k [columns, ndof]} of a case from the oracle's right-hand sides (bs: others) -- the global replica, or with `dist` (a
    `Dist0`) level 0 in the row-distributed form"""
    ks = case[-1] if ks is None else ks
    if case[0] == "emi":
        return {k: emi_xk(host, levels, case[2], k, dtype, b=None if bs is None else bs[0], mut=mut, dist=dist)[None] for k in ks}
    if case[4] is None:
        return {k: knp_xk(host, levels, k, dtype, bs=bs, blocks=case[2], mut=mut, dist=dist) for k in ks}
    return knp_xk(host, levels, tuple(ks), dtype, bs=bs, blocks=case[2], mut=mut, dist=dist, method=("gmres", case[4]), reverse=reverse)


def part_reference(host, levels, case, bs=None):
    """{k: (x64 [columns, ndof], bounds [columns], scales [columns])} of the GLOBAL replica: `bound` of the float64 run against the
    extended-precision one; GMRES: also of the float64 run with reversed sums (`gm_reference`)"""
    x64, xhp = part_xk(host, levels, case, bs=bs), part_xk(host, levels, case, hp_dtype(), bs=bs)
    more = [part_xk(host, levels, case, reverse=True, bs=bs)] if case[0] == "knp" and case[4] is not None else []
    return {k: (x64[k], [bound(x64[k][s], xhp[k][s], *[m[k][s] for m in more]) for s in range(len(x64[k]))],
                [float(np.abs(xhp[k][s]).max()) for s in range(len(x64[k]))]) for k in x64}


def hp_dtype():
    return HP if HP is not None else "fsum"


def bound(x64, xhp, *more64):
    """the comparison bound of DESIGN.md ("V-cycle parity"), measured on the reference itself: 32 times the rounding error of the
    float64 replica against the extended-precision one, at least 1e-13 of the result; above 1e-9 the case is ill-conditioned.
    more64: further float64 runs of the same replica (GMRES: the inner products summed from the other end); the largest error counts."""
    xhp = np.asarray(xhp)
    scale = float(np.abs(xhp).max())
    err = max(float(np.abs(np.asarray(x) - xhp).max()) for x in (x64,) + more64)
    bd = max(32.0 * err, 1e-13 * scale)
    assert bd <= 1e-9 * scale, "ill-conditioned case: bound %.3g of the result" % (bd / scale)
    return bd
