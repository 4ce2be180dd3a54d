"""CPU checks of the host replica of the auxiliary-space preconditioner (tests/amg_ref.py), the reference a comparison of the device's
k-iteration iterates is meant to use: the replica V-cycle is a symmetric positive operator that preconditions, it equals
P Ac^-1 P^T where that is what it must be, the hand-built hierarchies reach every instantiation of the density-dispatched kernels of csrc/amg_vcycle.hip, and each of six
deliberate errors in the replica moves the k-iteration result by at least 100 times the comparison bound (amg_ref.bound).
For the KNP solve on the drift-free class table of solve.hip (build_bj_table): the replica's table blocks are one block per table key,
to the bit; the two block sets give iterates at least 1e6 bounds apart; and the bound exists for every case the device runs.
For restarted GMRES (amg_ref.gmres): the replica minimises the residual over the stored Z_j, restarts exactly, every case the device
runs has its bound and reaches the passes of the inner products it is meant to, eight deliberate errors are far above the bound, and
the converged cases take every decision by a margin.
No GPU is needed, but knpemidg.amg builds its hierarchies with the host routines of the built library (as tests/test_host.py does)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as ar

_HOSTS = {}


def _host(names=None):
    if names not in _HOSTS:
        _HOSTS[names] = ar.Host("box_P1", names)
    return _HOSTS[names]


def _laplacian(n):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    return (sp.kron(sp.identity(n), T) + sp.kron(T, sp.identity(n)) + 0.01 * sp.identity(n * n)).tocsr()


def _cg(A, b, M, tol=1e-10, maxit=2000):
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    p, rho = z.copy(), r @ z
    for it in range(1, maxit + 1):
        w = A @ p
        alpha = rho / (p @ w)
        x += alpha * p
        r -= alpha * w
        if np.linalg.norm(r) <= tol * np.linalg.norm(b):
            return x, it
        z = M(r)
        rho, rho_old = r @ z, rho
        p = z + (rho / rho_old) * p
    return x, maxit


def test_replica_vcycle_is_a_symmetric_preconditioner(monkeypatch):
    from knpemidg import amg
    monkeypatch.setenv("KNP_AMG_MAXCOARSE", "20")
    monkeypatch.setenv("KNP_AMG_DEGREE", "2")
    A = _laplacian(30)
    levels = amg.build_hierarchy(A)
    assert len(levels) >= 3, [lv.A.shape[0] for lv in levels]
    H = ar.store(levels)
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
    Vx, Vy = ar.vcycle(H, x), ar.vcycle(H, y)
    assert abs(x @ Vy - y @ Vx) <= 1e-12 * max(abs(x @ Vy), abs(y @ Vx)), (x @ Vy, y @ Vx)
    assert x @ Vx > 0 and y @ Vy > 0
    # several columns: each one from its own right-hand side alone, to the bit
    XY = ar.vcycle(H, np.stack([x, y]))
    assert np.array_equal(XY[0], Vx) and np.array_equal(XY[1], Vy)
    b = rng.standard_normal(A.shape[0])
    dinv = 1.0 / A.diagonal()
    x_v, n_v = _cg(A, b, lambda r: ar.vcycle(H, r))
    x_j, n_j = _cg(A, b, lambda r: dinv * r)
    assert n_v < n_j and n_v < 40, (n_v, n_j)
    assert np.abs(x_v - x_j).max() <= 1e-7 * np.abs(x_j).max()
    # float64 and the extended-precision run agree to rounding
    hp = ar.vcycle(ar.store(levels, ar.hp_dtype()), x)
    assert np.abs(Vx - hp).max() <= 1e-13 * np.abs(Vx).max()
    # the fallback for machines without an 80-bit long double (exactly rounded row sums) is the same operator
    fs = ar.vcycle(ar.store(levels, "fsum"), x)
    assert np.abs(fs - hp).max() <= 1e-13 * np.abs(Vx).max()


def test_two_levels_without_smoothing_are_the_galerkin_correction():
    rng = np.random.default_rng(6)
    levels = ar.synthetic((120, 17), (9,), (4,), (0,), 3.0, 8)
    Ac = (levels[0].R @ levels[0].A @ levels[0].P).toarray()
    levels[1].pinv = np.linalg.inv(Ac)                                  # (float64: `store` rounds it as the device does)
    b = rng.standard_normal(120)
    P32 = levels[0].P.astype(np.float32).astype(np.float64)
    want = P32 @ (levels[1].pinv.astype(np.float32).astype(np.float64) @ (P32.T @ b))
    for dtype in (np.float64, ar.hp_dtype()):
        got = ar.vcycle(ar.store(levels, dtype), b)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # and with the unrounded inverse it inverts Ac on the range of P
    e = rng.standard_normal(17)
    assert np.abs(levels[1].pinv @ (Ac @ e) - e).max() < 1e-9


def test_hand_built_hierarchies_reach_every_kernel_instantiation():
    """by_density (csrc/amg_vcycle.hip) chooses G in {1, 4, 8, 64} by the average row length (<= 12, <= 40, <= 96, above:
    amg_ref.BANDS) and NC = 2 for an even column count; every synthetic hierarchy is meant to run with one column (EMI) and with two
    (KNP).  No combination is out of reach: k_csr<0> runs on R of every level above a transfer-only or the coarsest one and on P of a
    transfer-only level, k_csr_first on R above a smoothed level, the other four on A and P of smoothed levels."""
    assert "KNP_AMG_G4" not in os.environ                               # the library reads it once per process (g4_limit)
    h = _host()
    S = ar.synthetic_set(h.ncg, h.scale())
    got = set()
    assert set(S) == set(ar.SYNTHETIC)                                  # the list tests/test_gpu_amg.py runs with one and with two columns
    for name in ar.SYNTHETIC:
        got |= ar.launches(S[name], 1) | ar.launches(S[name], 2)
    want = {(k, g, nc) for k in ar.KERNELS for g in (1, 4, 8, 64) for nc in (1, 2)}
    assert len(want) == 48 and got == want, sorted(want - got)
    # k_cheb_step needs a smoothed level of degree >= 2 in every band; the top band needs its > 96 entries per row for real
    top = [lv for lv in S["bands"][:-1] if lv.A.nnz / lv.A.shape[0] > 96.0]
    assert top and top[0].A.shape[0] >= 130 and top[0].cheb_degree >= 2
    assert {lv.cheb_degree for name in ("bands", "bands_t0") for lv in S[name][:-1]} == {0, 1, 2, 3}
    # the production EMI hierarchy of this mesh stays in the two lowest bands: without the hand-built ones 24 instantiations never run
    prod = ar.launches(h.emi_levels(), 1)
    assert {g for _, g, _ in prod} <= {1, 4}, sorted(prod)


def _targets(levels, mutation, ncol):
    """where the mutation changes something: levels, or (level, matrix) pairs for drop_tail"""
    nl = len(levels)
    if mutation == "drop_tail":
        t = ar.drop_tail_targets(levels, ncol)
        assert {l for l, _ in t} == set(range(nl - 1)), ("a level without a row of length 1 modulo U G", t)
        return t
    if mutation == "dense_last_row":
        return [nl - 1]
    if mutation == "no_prolongation":
        return list(range(nl - 1))
    if mutation == "swap_columns":
        return list(range(nl))
    return [l for l in range(nl - 1) if levels[l].cheb_degree >= 1]     # a smoothed level: its A is used / it has a post-smoothing step


@pytest.mark.parametrize("cheb", [False, True])
@pytest.mark.parametrize("name", ar.SYNTHETIC)
def test_mutations_of_the_replica_are_far_above_the_bound(name, cheb):
    """(a) one level's A not rounded to fp32, (b) the last entry of the rows of length 1 modulo U G lost in one matrix of one level (every
    level, every matrix that has such rows), (d) one post-smoothing step short, (e) no x += P x_coarse, (f) the dense product without
    its last row: the EMI result x_3, with either DG smoother, moves by >= 100 bounds on every level where the error can be made."""
    h = _host()
    levels = ar.synthetic_set(h.ncg, h.scale())[name]
    x = ar.emi_xk(h, levels, cheb, 3)
    bd = ar.bound(x, ar.emi_xk(h, levels, cheb, 3, ar.hp_dtype()))
    for mutation in ar.MUTATIONS:
        if mutation == "swap_columns":
            continue
        ts = _targets(levels, mutation, 1)
        assert ts, (name, mutation)
        for t in ts:
            moved = np.abs(ar.emi_xk(h, levels, cheb, 3, mut=(mutation, t)) - x).max()
            assert moved >= 100.0 * bd, (name, mutation, t, moved / bd)


@pytest.mark.parametrize("name", ar.SYNTHETIC)
def test_column_mutations_of_the_replica_are_far_above_the_bound(name):
    """two species sharing the hierarchy (two interleaved columns, U = 2): (c) the columns' results swapped on one level, and (b) again
    with the row-length classes of the two-column kernels: the KNP result x_2 of every species moves by >= 100 bounds."""
    h = _host()
    levels = ar.synthetic_set(h.ncg, h.scale(knp=True))[name]
    x = ar.knp_xk(h, levels, 2)
    xhp = ar.knp_xk(h, levels, 2, ar.hp_dtype())
    bd = max(ar.bound(x[s], xhp[s]) for s in range(2))
    for mutation in ("swap_columns", "drop_tail"):
        for t in _targets(levels, mutation, 2):
            moved = np.abs(ar.knp_xk(h, levels, 2, mut=(mutation, t)) - x).max(axis=1)
            assert moved.min() >= 100.0 * bd, (name, mutation, t, moved / bd)


def test_one_hierarchy_per_species_and_more_ions():
    """three solved species (four ions), each with its own hierarchy: the replica's bound holds, the drift-dominated cells keep the
    per-cell blocks (Peclet number), exchanging two species' hierarchies or breaking one of them moves that species by >= 100 bounds
    and leaves the others' bits alone; four solved species (five ions) share one hierarchy as four columns."""
    names = ("K", "Cl", "X", "Na")
    h = _host(names)
    assert h.pb.N_ions == 3 and h.peclet() > 0.5
    S = ar.synthetic_set(h.ncg, h.scale(knp=True))
    per = [S["bands"], S["bands_t0"], S["coarse_2"]]
    x = ar.knp_xk(h, per, 2)
    xhp = ar.knp_xk(h, per, 2, ar.hp_dtype())
    bd = [ar.bound(x[s], xhp[s]) for s in range(3)]
    mixed = ar.knp_xk(h, [per[1], per[0], per[2]], 2)
    # (the spectral bound of the DG smoother is estimated jointly, from the same right-hand sides: species 2 keeps its bits)
    assert np.array_equal(mixed[2], x[2])
    assert all(np.abs(mixed[s] - x[s]).max() >= 100.0 * bd[s] for s in (0, 1))
    broken = ar.knp_xk(h, per, 2, mut=("no_prolongation", 0))
    assert all(np.abs(broken[s] - x[s]).max() >= 100.0 * bd[s] for s in range(3))
    h5 = _host(("K", "Cl", "X", "Y", "Na"))
    assert h5.pb.N_ions == 4 and h5.peclet() > 0.5
    S5 = ar.synthetic_set(h5.ncg, h5.scale(knp=True))
    y = ar.knp_xk(h5, S5["bands"], 2)
    yhp = ar.knp_xk(h5, S5["bands"], 2, ar.hp_dtype())
    swapped = ar.knp_xk(h5, S5["bands"], 2, mut=("swap_columns", 2))
    for s in range(4):
        moved = np.abs(swapped[s] - y[s]).max()
        assert (moved >= 100.0 * ar.bound(y[s], yhp[s])) == (s < 2), (s, moved)


@pytest.mark.parametrize("mesh", ["box_P1", "box_P2", "2D_P1"])
def test_emi_preconditioner_replica(mesh):
    """The additive EMI preconditioner z = S(r) + P_dg V(P_dg^T r) of the replica on the three meshes, production hierarchy: with the
    cell blocks as S it is the sum of its parts; with the two-step Chebyshev S (k_bj_cheb2's closed form) it equals two literal steps
    of the Chebyshev recurrence on Binv A; both are symmetric, as PCG needs; and the spectral bound the Chebyshev step rests on
    (bj_lambda_max: 20 power steps from b, times 1.1) lies between 0.9 and 1.1 of the spectral radius of Binv A."""
    import scipy.sparse.linalg as spla
    h = _HOSTS.setdefault(mesh, ar.Host(mesh)) if mesh != "box_P1" else _host()
    ref, levels = h.ref, h.emi_levels()
    H = ar.store(levels)
    n, nd = h.pb.ndof, h.nd
    Bsp = sp.block_diag(list(ref.binv_emi), format="csr")
    Pd = sp.csr_matrix((np.ones(n), (np.arange(n), h.dg2cg.ravel())), shape=(n, h.ncg))
    rng = np.random.default_rng(9)
    r, q = rng.standard_normal(n), rng.standard_normal(n)
    coarse = lambda v: Pd @ ar.vcycle(H, Pd.T @ v)
    M0 = ar.EmiPrecond(ref.A_emi, ref.binv_emi, h.dg2cg, H)
    want = Bsp @ r + coarse(r)
    assert np.abs(M0(r) - want).max() <= 1e-13 * np.abs(want).max()
    lmax = ar.bj_lambda_max([ref.A_emi], [ref.binv_emi], [ref.b_emi])
    true = abs(spla.eigs(Bsp @ ref.A_emi, k=1, which="LM", return_eigenvectors=False, tol=1e-8)[0])
    assert 0.9 * true <= lmax <= 1.1 * true * (1.0 + 1e-6), (lmax, true)
    M1 = ar.EmiPrecond(ref.A_emi, ref.binv_emi, h.dg2cg, H, lmax)
    L = ar._Level()                                                     # Chebyshev on Binv A: `smooth` with A <- Binv A, D <- I
    L.A, L.dinv, L.rho, L.cheb_lower, L.cheb_degree = (Bsp @ ref.A_emi).tocsr(), np.ones(n), lmax, ar.BJ_LMIN, 2
    want = ar.smooth(L, None, Bsp @ r, True) + coarse(r)
    assert np.abs(M1(r) - want).max() <= 1e-12 * np.abs(want).max()
    for M in (M0, M1):
        a, b = q @ M(r), r @ M(q)
        assert abs(a - b) <= 1e-9 * max(abs(a), abs(b)), (mesh, a, b)
    if mesh != "2D_P1":
        # k-iteration PCG with it, float64 against extended precision: a usable reference (the 2D mesh's single-level hierarchy is not:
        # its dense pseudo-inverse carries the 1e8 condition of the isolated subdomain-constant mode)
        for cheb in (False, True):
            ar.bound(ar.emi_xk(h, levels, cheb, 3), ar.emi_xk(h, levels, cheb, 3, ar.hp_dtype()))


# ---- the drift-free class table of the KNP solve (solve.hip: build_bj_table) ------------------------------------------------------------
_TABLE_HOSTS = {}


def _table_host(mesh, ns=2, materials=False):
    key = (mesh, ns, materials)
    if key not in _TABLE_HOSTS:
        _TABLE_HOSTS[key] = ar.Host(mesh, ar.IONS[ns], phi_scale=ar.TABLE_PHI_SCALE, materials=materials)
    return _TABLE_HOSTS[key]


@pytest.mark.parametrize("materials", [False, True])
@pytest.mark.parametrize("mesh", ["box_P1", "box_P2"])
def test_table_blocks_are_one_block_per_key(mesh, materials):
    """What lets a table stand for the cells: within every key (geometry class, material, facet kinds) the oracle's drift-free diagonal
    blocks, inverted and rounded to fp32, hold the same bits -- also with four materials and interior SIPG facets between different
    ones (the block takes the cell's own D only); with the drift they do not.  The keys fit build_bj_table's 8192 entries, and the
    potential of these cases is on the table's side of the switch (Peclet number <= 0.5) by a margin."""
    h = _table_host(mesh, materials=materials)
    keys = h.table_keys()
    ids = {}
    for c, key in enumerate(keys):
        ids.setdefault(key, []).append(c)
    assert 24 <= len(ids) <= 8192, len(ids)
    assert len({k[0] for k in ids}) == 24 and len({k[1] for k in ids}) == (4 if materials else 1)
    if materials:
        fc, D = h.mt[0].facet_cells[h.pb.int0], np.stack([ion["D"] for ion in h.pb.ions], axis=1)
        assert (D[fc[:, 0]] != D[fc[:, 1]]).any(axis=1).sum() >= 10
    tab, cell = h.knp_table_blocks(), h.knp()[1]
    assert len(tab) == h.pb.N_ions and tab[0].shape == (len(keys), h.nd, h.nd)
    spread = lambda B: max(np.abs(B[cs] - B[cs[0]]).max() / np.abs(B[cs[0]]).max() for cs in ids.values())
    for s in range(h.pb.N_ions):
        assert all(np.array_equal(tab[s][cs], np.broadcast_to(tab[s][cs[0]], tab[s][cs].shape)) for cs in ids.values()), (mesh, s)
        assert spread(tab[s]) == 0.0 and spread(cell[s]) > 1e-3, (spread(tab[s]), spread(cell[s]))
    assert 0.1 <= h.peclet() <= 0.4, h.peclet()


@pytest.mark.parametrize("materials", [False, True])
@pytest.mark.parametrize("mesh", ["box_P1", "box_P2"])
def test_table_and_cell_replicas_are_far_apart(mesh, materials):
    """the discriminating power of the device comparison on the table path: x_1 and x_2 with the drift-free blocks and with the per-cell
    blocks differ by >= 1e6 bounds for every species (measured: >= 1e9) -- a device on the other block set cannot pass"""
    h = _table_host(mesh, materials=materials)
    levels = ar.synthetic_set(h.ncg, h.scale(knp=True))["bands"]
    for k in (1, 2):
        xt = ar.knp_xk(h, levels, k, blocks="table")
        xc = ar.knp_xk(h, levels, k, blocks="cell")
        xhp = ar.knp_xk(h, levels, k, ar.hp_dtype(), blocks="table")
        for s in range(h.pb.N_ions):
            ratio = np.abs(xt[s] - xc[s]).max() / ar.bound(xt[s], xhp[s])
            print("TABLE/CELL %s materials=%d k=%d species %d: %.3g bounds" % (mesh, materials, k, s, ratio))
            assert ratio >= 1e6, (mesh, materials, k, s, ratio)


@pytest.mark.parametrize("mesh", ["box_P1", "box_P2"])
def test_one_wrong_table_index_is_far_above_the_bound(mesh):
    """a single cell that reads another entry of the table (the next cell's whose block differs: a wrong bj_idx, a wrong key) moves
    x_1 of every species by >= 1e6 bounds -- every 16th cell (measured over all cells: >= 4.7e9 on the P1 box, >= 9.1e9 on the P2 box)"""
    h = _table_host(mesh)
    levels = ar.synthetic_set(h.ncg, h.scale(knp=True))["bands"]
    tab = h.knp_table_blocks()
    nc = len(tab[0])
    x = ar.knp_xk(h, levels, 1, blocks="table")
    xhp = ar.knp_xk(h, levels, 1, ar.hp_dtype(), blocks="table")
    bd = [ar.bound(x[s], xhp[s]) for s in range(2)]
    for c in range(3, nc, 16):
        o = next(d % nc for d in range(c + 1, c + nc) if not np.array_equal(tab[0][d % nc], tab[0][c]))
        wrong = [t.copy() for t in tab]
        for t in wrong:
            t[c] = t[o]
        y = ar.knp_xk(h, levels, 1, blocks=wrong)
        moved = [np.abs(x[s] - y[s]).max() / bd[s] for s in range(2)]
        assert min(moved) >= 1e6, (mesh, c, o, moved)


@pytest.mark.parametrize("case", ar.TABLE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_table_cases_of_the_device_are_well_conditioned(case):
    """amg_ref.bound raises for an ill-conditioned case (bound above 1e-9 of the result): none of the cases the device runs is one"""
    mesh, ns, names, materials = case
    h = _table_host(mesh, ns, materials)
    S = ar.synthetic_set(h.ncg, h.scale(knp=True))
    levels = S[names] if isinstance(names, str) else [S[n] for n in names]
    for k in (1, 2):
        x64 = ar.knp_xk(h, levels, k, blocks="table")
        xhp = ar.knp_xk(h, levels, k, ar.hp_dtype(), blocks="table")
        for s in range(ns):
            bd = ar.bound(x64[s], xhp[s])
            print("TABLE BOUND %s k=%d species %d: %.3g" % (case, k, s, bd / np.abs(xhp[s]).max()))


def _apart(h, levels, k, bs, right, wrong, tag):
    """x_k of the replica by the rule (blocks, lmax) `right` and by `wrong`, in bounds of the right one; every species >= 1e6"""
    x = ar.knp_xk(h, levels, k, bs=bs, blocks=right[0], lmax=right[1])
    xhp = ar.knp_xk(h, levels, k, ar.hp_dtype(), bs=bs, blocks=right[0], lmax=right[1])
    y = ar.knp_xk(h, levels, k, bs=bs, blocks=wrong[0], lmax=wrong[1])
    ratio = [np.abs(x[s] - y[s]).max() / ar.bound(x[s], xhp[s]) for s in range(len(x))]
    print("SWITCH %s: %s bounds" % (tag, ", ".join("%.3g" % r for r in ratio)))
    assert min(ratio) >= 1e6, (tag, ratio)


def test_switch_cases_of_the_device_tell_the_rule_from_a_broken_one():
    """the device tests of the switch between the two block sets (tests/test_gpu_amg.py) compare with the replica by the rules of
    knp_knp_solve; here, what a broken rule would give instead -- the other block set, the array the table build left behind, a stale
    array or table, a spectral bound kept or re-estimated at the wrong solve -- is >= 1e6 bounds away in every step and species"""
    lo = _table_host("box_P1")
    levels = ar.synthetic_set(lo.ncg, lo.scale(knp=True))["bands"]
    bs = lo.knp()[2]
    other = {"table": "cell", "cell": "table"}
    for pe, blocks in ((0.45, "table"), (0.55, "cell")):
        for k in (1, 2):
            _apart(ar.at_peclet(lo, pe), levels, k, bs, (blocks, None), (other[blocks], None), "Peclet %.2f k=%d" % (pe, k))
    nc = lo.mt[0].num_cells()
    for mesh, cell in (("box_P1", 0), ("box_P1", nc - 1), ("box_P2", 323)):
        h0 = _table_host(mesh)
        lv = ar.synthetic_set(h0.ncg, h0.scale(knp=True))["bands"]
        _apart(ar.one_cell_peclet(h0, cell), lv, 1, h0.knp()[2], ("cell", None), ("table", None), "%s one cell %d" % (mesh, cell))
    for st in ar.switch_sequence(lo, bs):
        for what, wrong in st["wrong"].items():
            _apart(st["host"], levels, 1, bs, (st["blocks"], st["lmax"]), wrong, "step %s / %s" % (st["tag"], what))
    for what, h in (("dt", lo.variant(dt=lo.pb.dt / 2)), ("materials", lo.variant(D=ar.four_materials(lo.pb)))):
        _apart(h, levels, 1, bs, ("table", None), (lo.blocks("table"), None), "new %s / table of the old ones" % what)


# ---- the GMRES replica (amg_ref.gmres: krylov.hip gmres_impl, krylov_scalar.hpp gm_scalar_op) -----------------------------------------------
_GM_HOSTS, _GM_REF = {}, {}


def _gm_host(case):
    key = ar.gm_host_args(case)
    if key not in _GM_HOSTS:
        h = ar.Host(*key)
        _GM_HOSTS[key] = (h, ar.synthetic_set(h.ncg, h.scale(knp=True)))
    return _GM_HOSTS[key]


def _gm_ref(case):
    """amg_ref.gm_reference of a case of GM_CASES, computed once"""
    if case not in _GM_REF:
        h, S = _gm_host(case)
        _GM_REF[case] = ar.gm_reference(h, ar.gm_levels(S, case[2]), case[3], case[4], case[5])
    return _GM_REF[case]


_GM_ID = lambda c: "-".join(str(v) for v in c[:5])


@pytest.mark.parametrize("blocks", ["cell", "table"])
@pytest.mark.parametrize("mesh,name", [("box_P1", "coarse_257"), ("2D_P1", "mid")])
def test_gmres_replica_minimises_the_residual(mesh, name, blocks):
    """within one cycle x_k = x_0 + Z y with y the minimiser of ||r_0 - A Z y||_2 over the k stored Z_j = M^-1 V_j: the replica's y
    (Hessenberg matrix, rotations, back substitution) against the dense least-squares solution of LAPACK.  The extended-precision
    replica carries no error of its own at this level; the float64 least-squares solve has a relative error of about
    eps cond(A Z) (1 + cond(A Z) ||r_k|| / ||r_0||) in y (Golub & Van Loan, Matrix Computations, 5.3.7), and Z y is compared in
    units of ||Z||_2 ||y||_2: the tolerance is 10 eps cond(A Z)^2 of that."""
    case = (mesh, 2, name, blocks, 30, (4, 12))
    h, S = _gm_host(case)
    As, bs, M = ar._knp_system(h, S[name], ar.hp_dtype(), None, None, None, blocks, None)
    for k in case[5]:
        sys_, snap = ar.gmres_run(As, bs, M, k, 30, ar.hp_dtype(), snapshots=(k,))
        for s, st in enumerate(sys_):
            Z = np.stack([np.asarray(z, dtype=np.float64) for z in st.Z_done], axis=1)
            assert Z.shape[1] == k
            AZ = As[s] @ Z
            y, _, _, sv = np.linalg.lstsq(AZ, np.asarray(bs[s], dtype=np.float64), rcond=None)
            cond = sv[0] / sv[-1]
            tol = 10.0 * np.finfo(np.float64).eps * cond ** 2 * np.linalg.norm(Z, 2) * np.linalg.norm(y)
            diff = np.linalg.norm(np.asarray(snap[k][s], dtype=np.float64) - Z @ y)
            print("GMRES LSQ %s %s %s k=%d species %d: cond(A Z) %.3g, |x_k - Z y*| %.3g, tolerance %.3g" % (mesh, name, blocks, k, s, cond,
                                                                                                          diff, tol))
            assert tol <= 1e-6 * np.linalg.norm(snap[k][s].astype(np.float64)), "the tolerance says nothing on this case"
            assert diff <= tol, (mesh, name, blocks, k, s, diff / tol)


def test_gmres_replica_restarts_from_the_true_residual():
    """k > m iterations of GMRES(m) are k - m iterations started from x_m, to the bit (the residual b - A x_m is all a cycle hands on)"""
    case = ar.GM_CASES[1]
    h, S = _gm_host(case)
    As, bs, M = ar._knp_system(h, S[case[2]], np.float64, None, None, None, case[3], None)
    for m, k in ((30, 33), (3, 7), (8, 20)):
        whole = ar.gmres(As, bs, M, k, m)
        xm = ar.gmres(As, bs, M, m * ((k - 1) // m), m)
        again = ar.gmres(As, bs, M, k - m * ((k - 1) // m), m, x0=xm)
        assert np.array_equal(whole, again), (m, k)
        assert not np.array_equal(whole, xm)


def test_gmres_snapshots_are_the_shorter_solves():
    """one run to the largest count returns every listed count's iterate: the bits of a run that ends there"""
    case = ar.GM_CASES[1]
    h, S = _gm_host(case)
    As, bs, M = ar._knp_system(h, S[case[2]], np.float64, None, None, None, case[3], None)
    snap = ar.gmres(As, bs, M, (2, 10, 30, 33), 30)
    for k in (2, 10, 30, 33):
        assert np.array_equal(snap[k], ar.gmres(As, bs, M, k, 30)), k


@pytest.mark.parametrize("case", ar.GM_CASES, ids=_GM_ID)
def test_gmres_cases_of_the_device_are_well_conditioned(case):
    """amg_ref.bound raises above the cap of 1e-9: every case, count and species the device runs has its bound (none is skipped)"""
    ref = _gm_ref(case)
    assert sorted(ref) == sorted(case[5])
    for k, (x, bds, scales) in ref.items():
        assert len(bds) == case[1]
        for s in range(case[1]):
            assert 1e-13 * scales[s] <= bds[s] <= 1e-9 * scales[s]
            print("GMRES BOUND %s k=%d species %d: %.3g" % (_GM_ID(case), k, s, bds[s] / scales[s]))


def test_gmres_cases_reach_every_pass_of_the_inner_products():
    """what the counts of GM_CASES reach, per block set: columns whose inner products take two, three and four passes of k_gm_dots
    with a partial last pass, the full cycle of 30 columns and a restart behind it; restarts of short cycles (m = 3, m = 8) that end
    in an unfinished cycle; two and three species, one hierarchy per species, all three meshes"""
    for blocks in ("cell", "table"):
        cases = [c for c in ar.GM_CASES if c[3] == blocks]
        full = [c for c in cases if c[:2] == ("box_P1", 2) and isinstance(c[2], str) and c[4] == 30]
        assert full
        for c in full:
            last = {ar.gm_batches(ar.gm_columns(k, 30)[-1]) for k in c[5]}
            assert {(1, True), (2, True), (3, True), (4, True)} <= last, (c, last)
            assert 30 in c[5] and max(c[5]) > 30 and 0 < max(c[5]) % 30 < 8
        assert {c[1] for c in cases} >= {2, 3} and any(not isinstance(c[2], str) for c in cases)
        assert {c[0] for c in cases} >= {"box_P1", "box_P2"}
    assert any(c[0] == "2D_P1" for c in ar.GM_CASES)
    short = {(c[4], k) for c in ar.GM_CASES if c[4] < 30 for k in c[5]}
    assert {m for m, _ in short} == {3, 8} and all(k > m and k % m for m, k in short)
    assert any(k > 2 * m for m, k in short)


@pytest.mark.parametrize("mutation", ar.GM_MUTATIONS)
def test_gmres_mutations_of_the_replica_are_far_above_the_bound(mutation):
    """each deliberate error of the replica -- the inner products of columns >= 8 lost; the one partial pass of k_gm_dots lost; the
    first rotation not applied to the new column; the new basis vector not normalised; the update taken from V instead of Z; back
    substitution over k - 1 columns; the first two species' y exchanged; the restart's residual taken from x without the cycle's
    update -- moves x_k by >= 100 bounds for every species on a listed case of either block set: a device with that defect cannot pass"""
    for blocks in ("cell", "table"):
        case = next(c for c in ar.GM_CASES if c[3] == blocks and c[5] == ar.GM_KS)
        h, S = _gm_host(case)
        ref = _gm_ref(case)
        worst = {}
        for k in (17, 33):
            wrong = ar.knp_xk(h, S[case[2]], k, blocks=blocks, method=("gmres", 30), mut=mutation)
            x, bds, _ = ref[k]
            worst[k] = min(np.abs(wrong[s] - x[s]).max() / bds[s] for s in range(case[1]))
        print("GMRES MUTATION %s %s: %s bounds" % (mutation, _GM_ID(case), ", ".join("k=%d %.3g" % kv for kv in worst.items())))
        assert max(worst.values()) >= 100.0, (mutation, blocks, worst)


@pytest.mark.parametrize("case", ar.GM_FREE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_gmres_free_running_cases_decide_by_a_margin(case):
    """the converged solves the device is compared with: every decision (estimate against T2, true residual against the tolerance) is
    >= 1e-3 of its threshold away from flipping in float64, with reversed sums and in extended precision, and the three runs count
    the same iterations and cycles (asserted by gm_free_reference) -- rounding on the device cannot change the path"""
    name, rtol, m = case
    h, S = _gm_host(("box_P1", 2, name, "table"))
    runs, bds, scales, margin = ar.gm_free_reference(h, S[name], rtol, m)
    print("GMRES FREE %s rtol %g m=%d: cycles %s, margin %.3g, bounds %s" % (name, rtol, m, [r["cycles"] for r in runs], margin,
                                                                             ["%.3g" % (b / s) for b, s in zip(bds, scales)]))
    assert margin >= 1e-3, margin
    assert all(sum(r["cycles"]) == r["niter"] and max(r["cycles"]) <= m for r in runs)
    _GM_REF[("free",) + case] = [r["cycles"] for r in runs]


def test_gmres_free_running_cases_cover_the_lockstep():
    """among the converged cases: one where the species end a shared cycle at different columns before column m (each by its own
    estimate; the earlier one idles), one where one species converges cycles before the other, and one with both"""
    cyc = {}
    for case in ar.GM_FREE_CASES:
        key = ("free",) + case
        if key not in _GM_REF:
            h, S = _gm_host(("box_P1", 2, case[0], "table"))
            _GM_REF[key] = [r["cycles"] for r in ar.gm_free_reference(h, S[case[0]], case[1], case[2])[0]]
        cyc[case] = _GM_REF[key]
    m_of = lambda case: case[2]
    shared_differ = [c for c, (a, b) in cyc.items() if any(x != y and max(x, y) < m_of(c) for x, y in zip(a, b))]
    sooner = [c for c, (a, b) in cyc.items() if abs(len(a) - len(b)) >= 2]
    assert shared_differ and sooner, cyc
    assert any(len(a) != len(b) and min(len(a), len(b)) >= 1 and (a[-1] < m_of(c) or b[-1] < m_of(c)) and max(len(a), len(b)) >= 2
               for c, (a, b) in cyc.items()), cyc


# ---- the row-distributed level 0 of a partitioned run (amg_ref.vcycle_dist0; tests/test_gpu_amg_partition.py) ---------------------------
_PART_HOSTS, _PART_REF, _PART_DIST = {}, {}, {}


@pytest.fixture
def part_env(monkeypatch):
    monkeypatch.setenv("KNP_AMG_MAXCOARSE", ar.PART_MAXCOARSE)
    for key in ("KNP_AMG_DEGREE0_EMI", "KNP_AMG_DEGREE0_KNP", "KNP_AMG_DEGREE0"):
        monkeypatch.delenv(key, raising=False)


def _part_ref(mesh, case):
    """(host, production hierarchy, amg_ref.part_reference) of a case, computed once"""
    key = ar.part_host_key(mesh, case)
    if (key, case) not in _PART_REF:
        if key not in _PART_HOSTS:
            _PART_HOSTS[key] = ar.Host(*key)
        h = _PART_HOSTS[key]
        levels = ar.part_levels(h, case)
        _PART_REF[(key, case)] = (h, levels, ar.part_reference(h, levels, case))
    return _PART_REF[(key, case)]


def _part_dist(host, pname):
    key = (id(host), pname)
    if key not in _PART_DIST:
        _PART_DIST[key] = ar.Dist0(host, ar.part_partition(host.mt[0], pname).owner)
    return _PART_DIST[key]


@pytest.mark.parametrize("group,pname", ar.PART_LAUNCHES, ids=lambda v: str(v))
def test_partitioned_cases_have_their_bounds_and_the_distributed_replica_is_the_global_one(part_env, group, pname):
    """every case the partitioned device runs (amg_ref.PART_GROUPS) has its bound -- amg_ref.bound raises above 1e-9 of the result --,
    and with level 0 in the row-distributed form of the case's partition (every rank's share of the global matrix rounded to fp32 on
    its own, right-hand sides as the ranks' partial sums, shared dofs summed over their owners in rank order, the level-1 right-hand
    side summed over the ranks) the replica's x_k stays within that bound of the global replica's: the global replica is the
    reference of the partitioned device.  (Measured: at most 0.64 bounds, EMI on the P1 box with the Chebyshev DG smoother, k = 3.)"""
    _, mesh, dist0, parts = ar.part_group(group)
    for case in parts[pname]:
        h, levels, ref = _part_ref(mesh, case)
        assert sorted(ref) == sorted(case[-1])
        assert [lv.A.shape[0] for lv in levels] == ([267, 52] if mesh == "box_P1" else [679, 124, 26])
        xd = ar.part_xk(h, levels, case, dist=_part_dist(h, pname)) if dist0 else None
        for k, (x64, bds, scales) in ref.items():
            for s in range(len(bds)):
                assert 1e-13 * scales[s] <= bds[s] <= 1e-9 * scales[s]
                moved = np.abs(xd[k][s] - x64[s]).max() / bds[s] if dist0 else 0.0
                print("PART BOUND %s %s %s k=%d column %d: %.3g, distributed replica %.3g bounds away" % (group, pname, ar.part_case_id(case),
                                                                                                        k, s, bds[s] / scales[s], moved))
                assert moved <= 1.0, (group, pname, case, k, s, moved)


def test_quadrant_partition_reaches_the_sums_of_three_and_four_owners(part_env):
    """what the partitions of the comparison reach: on the quadrants, conforming dofs with four owners on the P1 box and with two,
    three and four on the P2 box, interface peers that are no halo peers; on the slabs at most two owners; and a transfer-only level 0
    exchanges nothing (its mutations of the exchange cannot show: the degree-0 cases check the all-reduced level-1 right-hand side)"""
    for mesh, want in (("box_P1", {1, 2, 4}), ("box_P2", {1, 2, 3, 4})):
        h = _part_ref(mesh, ("emi", 1 if mesh == "box_P1" else None, False, (1, 2, 3)))[0]
        d0 = _part_dist(h, "quad4")
        assert set(np.unique(d0.owners())) == want
        part = ar.part_partition(h.mt[0], "quad4")
        assert all(len(t[0]) == 3 for t in d0.tabs) and any(len(part.local(r).peers) == 2 for r in range(4))
        assert max(np.diff(t[3]).max() for t in d0.tabs) == 4               # k_if_add: up to four terms
        assert set(np.unique(_part_dist(h, "slab2").owners())) == {1, 2}


# distance of x_k from the correct distributed replica, in bounds, smallest over the columns and the counts of the case, measured on
# the quadrant partition (EMI: k = 1, 2, 3; KNP: k = 1, 2); 0: the error cannot show on that case
_DIST_MEASURED = {
    #                          EMI P1 deg 1  EMI P1 deg 2  EMI P2     KNP P1 3 species  KNP P1 4 species  KNP P2 2 species
    "two_owners":               (8.2e9,       2.5e9,        1.1e9,     4.5e10,           3.0e10,           3.5e10),
    "no_step_accumulation":     (0.0,         6.0e8,        2.0e9,     0.0,              0.0,              1.3e11),
    "zero_guess_unaccumulated": (2.0e9,       7.8e7,        6.5e8,     4.3e10,           5.6e10,           1.1e11),
    "rank_missing_level1":      (4.2e8,       1.5e8,        2.1e9,     8.5e10,           5.3e11,           7.3e10),
    "message_interleave":       (0.0,         0.0,          0.0,       7.9e10,           2.0e12,           1.7e11),
    "peer_offset":              (8.2e9,       2.5e9,        1.2e9,     1.5e11,           8.2e11,           1.6e11),
}
_DIST_CASES = (("box_P1", ("emi", 1, False, (1, 2, 3))), ("box_P1", ("emi", 2, False, (1, 2, 3))), ("box_P2", ("emi", None, False, (1, 2, 3))),
               ("box_P1", ("knp", 3, "cell", 1, None, (1, 2))), ("box_P1", ("knp", 4, "table", 1, None, (1, 2))),
               ("box_P2", ("knp", 2, "cell", None, None, (1, 2))))


@pytest.mark.parametrize("mutation", ar.DIST_MUTATIONS)
def test_mutations_of_the_distributed_replica_are_far_above_the_bound(part_env, mutation):
    """Deliberate errors of the row-distributed form, on the quadrant partition (dofs with three and four owners, three interface
    peers): the third and later owners of a shared dof left out of its sum; A d of the extra Chebyshev step not accumulated; the
    zero-guess smoother on the un-accumulated b; the last rank's part missing from the level-1 right-hand side; the columns of a
    message read in the wrong interleave; a peer's message read at the offset of its message to another rank.  Distance of x_k from
    the correct distributed replica in bounds of the case, smallest over columns and counts (_DIST_MEASURED, measured on the CPU):

      error                      EMI P1 deg 1  EMI P1 deg 2  EMI P2   KNP P1, 3 sp.  KNP P1, 4 sp.  KNP P2, 2 sp.
      two_owners                 8.2e9         2.5e9         1.1e9    4.5e10         3.0e10         3.5e10
      no_step_accumulation       0             6.0e8         2.0e9    0              0              1.3e11
      zero_guess_unaccumulated   2.0e9         7.8e7         6.5e8    4.3e10         5.6e10         1.1e11
      rank_missing_level1        4.2e8         1.5e8         2.1e9    8.5e10         5.3e11         7.3e10
      message_interleave         0             0             0        7.9e10         2.0e12         1.7e11
      peer_offset                8.2e9         2.5e9         1.2e9    1.5e11         8.2e11         1.6e11

    Asserted: a tenth of each.  The zeros are by construction: a level 0 of degree 1 has no extra Chebyshev step (the P1 cases of
    degree 2 and the P2 box, whose top level has degree 2, run it), and with one column a message has one interleave.  Every error is
    >= 1e7 bounds away on a case the device runs, with three and with four columns for the column error."""
    shown = 0
    for (mesh, case), measured in zip(_DIST_CASES, _DIST_MEASURED[mutation]):
        h, levels, ref = _part_ref(mesh, case)
        d0 = _part_dist(h, "quad4")
        x, y = ar.part_xk(h, levels, case, dist=d0), ar.part_xk(h, levels, case, dist=d0, mut=(mutation, 0))
        moved = min(np.abs(y[k][s] - x[k][s]).max() / ref[k][1][s] for k in ref for s in range(len(ref[k][1])))
        print("DIST MUTATION %s %s %s: %.3g bounds" % (mutation, mesh, ar.part_case_id(case), moved))
        if measured == 0.0:
            assert moved == 0.0, (mutation, mesh, case, moved)
        else:
            assert moved >= 0.1 * measured, (mutation, mesh, case, moved, measured)
            shown += moved >= 1e7
    assert shown >= 3, (mutation, shown)


def test_sub_assembled_level0_matrices_do_not_survive_the_fp32_rounding(part_env):
    """why Dist0Space.localize splits the GLOBAL matrix entry by entry: the ranks' matrices assembled from their own elements
    (Dist0Space.local_matrix) add up to the global one in float64, but the device rounds every rank's values to fp32 on their own, and
    a coupling between two shared dofs is then fl32(a_1) + fl32(a_2), not fl32(a_1 + a_2).  With them the distributed replica's x_k
    (EMI, P1 box, quadrants) is 2680 / 651 / 700 bounds (k = 1, 2, 3) from the global replica -- asserted: a tenth; with the split
    it is within the bound (the test above).  Tried once on the MI355X with the sub-assembled matrices: the device missed the bound of
    the global replica by 2677 / 652 / 700 bounds (plain DG smoother) and 2.0e4 / 1970 / 2831 (Chebyshev) -- the numbers of this replica."""
    case = ("emi", 1, False, (1, 2, 3))
    h, levels, ref = _part_ref("box_P1", case)
    d0 = _part_dist(h, "quad4")
    n = levels[0].A.shape[0]
    S = [sp.csr_matrix((np.ones(d.n), (np.arange(d.n), d.verts)), shape=(d.n, n)) for d in d0.D]
    r32 = lambda M: sp.csr_matrix((M.data.astype(np.float32).astype(np.float64), M.indices, M.indptr), shape=M.shape)
    A32 = r32(sp.csr_matrix(levels[0].A))
    split = sum(s.T @ r32(d.split_matrix(levels[0].A)) @ s for s, d in zip(S, d0.D))
    assert abs(split - A32).max() == 0.0                                # exact: every entry lives on one rank
    sub = sum(s.T @ r32(a) @ s for s, a in zip(S, d0.emi_matrices()))
    assert abs(sum(s.T @ a @ s for s, a in zip(S, d0.emi_matrices())) - levels[0].A).max() <= 1e-12 * abs(levels[0].A).max()
    assert 1e-9 * abs(A32).max() <= abs(sub - A32).max() <= 1e-7 * abs(A32).max()
    x = ar.part_xk(h, levels, case, dist=(d0, d0.emi_matrices()))
    for k, measured in zip((1, 2, 3), (2680.0, 651.0, 700.0)):
        moved = np.abs(x[k][0] - ref[k][0][0]).max() / ref[k][1][0]
        print("SUB-ASSEMBLED k=%d: %.3g bounds" % (k, moved))
        assert moved >= 0.1 * measured, (k, moved)
