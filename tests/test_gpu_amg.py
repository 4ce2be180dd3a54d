"""Every kernel variant of the AMG V-cycle (csrc/amg_vcycle.hip, csrc/amg_restrict.hip) and the transfer / smoother kernels around it
(csrc/krylov.hip) against the host replica tests/amg_ref.py, vector by vector.

The observable is the iterate x_k the device returns after k Krylov iterations from x_0 = 0 at a tolerance it cannot reach (status -3,
KnpError "did not converge": the documented contract): a deterministic function of b, the operator and the preconditioner.  PCG (EMI,
k = 1, 2, 3) applies the preconditioner k times, BiCGStab (KNP, k = 1, 2) 2 k times; everything past the first application runs the
per-iteration path (fused restrictions, k_restrict_sum with the fused first update, the replayed V-cycle graph, k_prolong_dot /
k_prolong_add(_pair)).  Hierarchies are uploaded through Device.amg_upload: the hand-built ones of amg_ref.synthetic_set reach all 48
instantiations of the density-dispatched kernels (tests/test_amg_ref_host.py asserts that) and coarsest levels of 1 ... 2051 rows; the
production ones come from amg.build_emi_levels.  The host runs the same iterations on the oracle's matrices with the fp32 cell blocks.

The KNP solve has two sets of cell blocks (solve.hip: knp_knp_solve): the per-cell inverses with the drift, and, on structured 3D meshes
while the cell Peclet number of the potential is at most 0.5 -- every production step -- the drift-free table of build_bj_table, one
block per (geometry class, material, facet kinds) that all Krylov vector kernels read through bj_block().  The synthetic potential has
Peclet number 5.4 (per-cell blocks); the "table" groups below run at 0.05 times that potential (0.27), with one and with four
materials, against the replica on the oracle's blocks assembled at phi = 0; the "switch" groups check which set a solve uses: on either
side of the limit, with the largest cell Peclet number at the edges of k_cell_peclet's waves and workgroups, through a fall-back and
return on a potential that changes on the device (one solve late, with the rebuilt per-cell array and the re-estimated spectral bound),
and after set_params.  Against the replica on the OTHER block set the table cases miss by 7.4e8 ... 6.5e11 bounds (tried once on the
MI355X; tests/test_amg_ref_host.py asserts >= 1e6 between the two replicas).

Restarted GMRES (knp_set_knp_krylov; gmres_impl, gm_scalar_op) is compared in the same way, with amg_ref.gmres: x_k of GMRES(m) for the
counts of amg_ref.GM_CASES -- with m = 30, k = 9 / 10, 17 and 25 end in the second, third and fourth pass of k_gm_dots with a partial
last pass, 30 is the full cycle, 33 the first restart; m = 3 and m = 8 restart in unfinished cycles -- on both block sets, with two and
three species, a shared hierarchy and one per species, on the three meshes; and solves run to convergence against amg_ref.gmres_free
(cycle ends on KS_GM_T2 at different columns, a species that idles or has converged cycles before the other, the joint restart): the
iteration counts are the replica's, the iterates within the bound, res[:, 1] is the host's norm of the returned iterate's residual.
A single Gram-Schmidt pass is more sensitive to the summation order than the short recurrences, so the GMRES bound takes the larger
error of two float64 runs of the replica (inner products summed from either end) against the extended-precision one.  Each of eight
deliberate errors of the replica (amg_ref.GM_MUTATIONS) is >= 9e7 bounds away on these cases (tests/test_amg_ref_host.py).

Bound ("V-cycle parity"): max(32 ||x64 - x_hp||_inf, 1e-13 ||x_hp||_inf) with x64 / x_hp the replica in float64 / extended
precision -- never taken from the device's numbers.  Measured on the MI355X, as multiples of ||x_k||_inf, worst case of each group:

  group                                                        largest bound   largest device error   worst error / bound
  ----------------------------------------------------------------------------------------------------------------------
  EMI  3D P1 box, 11 synthetic hierarchies, k = 1..3             4.7e-12         2.6e-13                0.08
  EMI  3D P1 box, production (one level)                         2.2e-10         6.6e-12                0.03
  EMI  3D P2 box, bands / bands_t0 / coarse_257                  1.0e-12         4.2e-14                0.08
  EMI  3D P2 box, production (two levels)                        7.1e-10         3.8e-11                0.05
  EMI  2D P1, bands / bands_t0 / coarse_257                      2.5e-13         1.2e-14                0.09
  KNP  3D P1 box, 2 species shared, 11 synthetic, k = 1, 2       1.0e-11         3.2e-13                0.18
  KNP  3D P1 box, 3 species shared                               1.2e-11         5.9e-13                0.19
  KNP  3D P1 box, 4 species shared                               8.4e-13         3.8e-14                0.23
  KNP  3D P1 box, one hierarchy per species (2 and 3 species)    1.2e-11         5.9e-13                0.35
  KNP  3D P2 box, 2 / 3 species shared                           1.8e-10         7.0e-12                0.20
  KNP  3D P2 box, one hierarchy per species                      1.4e-10         7.1e-12                0.22
  KNP  table, 3D P1 box, 2 species, 3 hierarchies + unfused      3.3e-11         1.8e-12                0.25
  KNP  table, 3D P1 box, 2 species shared, four materials        2.2e-12         1.0e-13                0.07
  KNP  table, 3D P1 box, 3 and 4 species shared                  3.3e-13         1.9e-14                0.14
  KNP  table, 3D P1 box, one per species, four materials         2.2e-12         6.4e-13                0.29
  KNP  table, 3D P2 box, bands / coarse_257                      1.8e-10         6.3e-12                0.20
  KNP  table, 3D P2 box, bands_t0, four materials                6.8e-11         1.5e-12                0.12
  KNP  switch, threshold (Peclet 0.45 table, 0.55 per cell)      8.0e-12         2.4e-13                0.21
  KNP  switch, largest Peclet number in 6 + 1 cell positions     1.1e-12         5.8e-14                0.27
  KNP  switch, fall-back and return on the device, 8 solves      3.7e-13         2.2e-14                0.12
  KNP  switch, table after set_params (dt / 2, four materials)   3.7e-13         2.2e-14                0.11
  GMRES(30)  3D P1 box, 2 species, per-cell blocks, 8 counts     8.8e-12         7.4e-13                0.20
  GMRES(30)  table, 3D P1 box, 2 species, 2 hierarchies, 8 counts 1.6e-11        1.6e-12                0.11
  GMRES(3), GMRES(8)  table, 3D P1 box, 2 species               5.4e-12         5.0e-13                0.11
  GMRES(30)  3D P1 box, 3 species shared (cell / table)          9.3e-13         2.8e-14                0.18
  GMRES(30)  3D P1 box, one hierarchy per species (cell / table) 2.5e-11         8.1e-13                0.11
  GMRES(30)  3D P2 box (cell / table), 2D P1 (cell)              6.2e-11         2.8e-12                0.07
  GMRES(30), GMRES(8)  converged solves, table, 6 cases          1.3e-11         5.4e-13                0.10
  (both DG smoothers, the random right-hand side and the unfused paths are inside their groups)

Two production cases are ill-conditioned by the rule above and are not run: the single-level hierarchy of the 2D mesh (bounds 0.85e-9 ...
7.3e-9) and x_3 on the P2 box with the plain cell blocks (1.2e-9; x_1 and x_2 of that case, 4.1e-11 and 5.9e-10, are run).

Each case also solves twice (same bits: graph replay, swapped x / d1 buffers) and, with several columns, changes one species'
right-hand side (the others' iterates keep their bits).  The eager V-cycle (KNP_NO_GRAPH, read once per process; what runs whenever
capture fails) has a child process of its own: same bound, and the bits of the graph replay."""
import contextlib

import numpy as np
import pytest

import amg_ref as ar
from common import device_for, push_state, set_params_of

pytestmark = pytest.mark.gpu

_CTX = {}
SMALL = ("bands", "bands_t0", "coarse_257")
ALL = ar.SYNTHETIC                 # the list whose coverage of the 48 kernel instantiations tests/test_amg_ref_host.py asserts


class Ctx:
    def __init__(self, mesh, names, phi_scale=1.0, materials=False):
        from knpemidg import _abi as A
        self.A = A
        self.host = ar.Host(mesh, names, phi_scale, materials)
        pb = self.host.pb
        self.dev = device_for(pb)
        push_state(self.dev, pb)
        self.dev.update_kappa()
        self.dev.emi_rhs()
        self.dev.update_dnphi()
        self.dev.knp_rhs()
        self.b_emi = self.dev.download(A.F_B_EMI)
        self.b_knp = self.dev.download(A.F_B_KNP).reshape(pb.N_ions, -1)
        self.ns = pb.N_ions
        self._sets = {}
        # the oracle's loads are the device's to rounding: a mismatch here is not a V-cycle error
        assert np.abs(self.b_emi - self.host.ref.b_emi).max() <= 1e-10 * np.abs(self.b_emi).max()

    def levels(self, name, knp=False):
        if knp not in self._sets:
            self._sets[knp] = ar.synthetic_set(self.host.ncg, self.host.scale(knp))
            self._sets[knp]["production"] = self.host.emi_levels() if not knp else None
        return self._sets[knp][name]

    def fail_solve(self, fn):
        with pytest.raises(self.A.KnpError, match="did not converge"):
            fn()

    def emi(self, k, b):
        A, dev = self.A, self.dev
        dev.upload(A.F_B_EMI, b)
        dev.upload(A.F_PHI, np.zeros(self.host.pb.ndof))               # x_0 = 0; also drops the extrapolation history
        self.fail_solve(lambda: dev.emi_solve(1e-30, maxit=k, check_every=1))
        return dev.download(A.F_PHI)

    def knp(self, k, b, keep_bound=False):
        """keep_bound: x_0 = 0 without a state upload, so that the spectral bound of the DG smoother (estimated from the right-hand side
        after every upload of c) stays the one of the previous solve"""
        A, dev = self.A, self.dev
        dev.upload(A.F_B_KNP, b)
        zero = np.zeros(self.ns * self.host.pb.ndof)
        if keep_bound:
            dev.upload(A.F_X, zero)
            dev.copy_field(A.F_C, A.F_X)
        else:
            dev.upload(A.F_C, zero)
        self.fail_solve(lambda: dev.knp_solve(1e-30, maxit=k, min_it=0, check_every=1))
        return dev.download(A.F_C).reshape(self.ns, -1)


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for c in _CTX.values():
        c.dev.close()
    _CTX.clear()


def _ctx(mesh, names=None, phi_scale=1.0, materials=False):
    key = (mesh, names, phi_scale, materials)
    if key not in _CTX:
        _CTX[key] = Ctx(*key)
    return _CTX[key]


def _report(tag, k, bd, err, scale):
    print("AMGPAR %-58s k=%d bound %.2e err %.2e" % (tag, k, bd / scale, err / scale))


def _check_emi(c, name, cheb, random_b=False, ks=(1, 2, 3)):
    levels = c.levels(name)
    b = c.b_emi
    if random_b:
        b = np.abs(b).max() * np.random.default_rng(31).uniform(-1.0, 1.0, size=b.shape)
    c.dev.emi_residual_target(0.0)
    c.dev.amg_upload(0, c.host.dg2cg, levels)
    c.dev.set_emi_dg_smoother(cheb)
    try:
        got = {k: (c.emi(k, b), c.emi(k, b)) for k in ks}
    finally:
        c.dev.set_emi_dg_smoother(None)
        c.dev.amg_clear(0)
        c.dev.upload(c.A.F_B_EMI, c.b_emi)
    bad = []
    for k, (x, again) in got.items():
        assert np.array_equal(x, again), (name, k, "a second identical solve gave other bits")
        x64 = ar.emi_xk(c.host, levels, cheb, k, b=b)
        xhp = ar.emi_xk(c.host, levels, cheb, k, ar.hp_dtype(), b=b)
        bd, err = ar.bound(x64, xhp), np.abs(x - x64).max()
        _report("emi %s %s cheb=%d%s" % (c.host.mesh_name, name, cheb, " random b" if random_b else ""), k, bd, err, np.abs(xhp).max())
        if not err <= bd:
            bad.append((k, err / bd))
    assert not bad, (name, cheb, bad)


@pytest.mark.parametrize("cheb", [False, True])
@pytest.mark.parametrize("name", ALL + ("production",))
def test_emi_iterates_box_p1(hip_lib, name, cheb):
    _check_emi(_ctx("box_P1"), name, cheb)


# (no production hierarchy on the 2D mesh: it is a single level of 252 dofs whose dense pseudo-inverse carries the 1e8 condition of
# the isolated subdomain-constant mode -- the float64 and extended-precision replicas themselves differ by 3e-11 ... 2e-10 of x_k
# there, 32 times that is 0.85e-9 ... 7.3e-9, above the 1e-9 at which a case counts as ill-conditioned)
@pytest.mark.parametrize("cheb", [False, True])
@pytest.mark.parametrize("mesh,name", [("box_P2", n) for n in SMALL + ("production",)] + [("2D_P1", n) for n in SMALL])
def test_emi_iterates_other_meshes(hip_lib, mesh, name, cheb):
    # (x_3 of the P2 production hierarchy with the plain cell blocks: the reference's own error puts the bound at 1.2e-9 of x_3)
    _check_emi(_ctx(mesh), name, cheb, ks=(1, 2) if (mesh, name, cheb) == ("box_P2", "production", False) else (1, 2, 3))


@pytest.mark.parametrize("cheb", [False, True])
def test_emi_iterates_random_right_hand_side(hip_lib, cheb):
    _check_emi(_ctx("box_P1"), "bands", cheb, random_b=True)


@pytest.mark.parametrize("switch,cheb", [("KNP_FUSE_FIRST0", False), ("KNP_FUSE_FIRST0", True), ("KNP_FUSE_CG_RESTRICT", False),
                                         ("KNP_FUSE_RESTRICT", True)])
@pytest.mark.parametrize("name", ["bands", "bands_t0"])
def test_emi_iterates_unfused_paths(hip_lib, monkeypatch, name, switch, cheb):
    """the three fusions are on by default (the tests above); here each one off (read per upload / per call)"""
    monkeypatch.setenv(switch, "0")
    _check_emi(_ctx("box_P1"), name, cheb)


# ---- KNP ---------------------------------------------------------------------------------------------------------------------------
IONS = ar.IONS


def _check_knp(c, names, independent=True, blocks="cell"):
    """names: one hierarchy shared by the species (slot 1, one column each) or a tuple with one per species (slots 1 ...)"""
    if blocks == "cell":
        assert c.host.peclet() > 0.5                                    # per-cell block inverses with the drift, as the replica's
    else:
        assert c.host.peclet() <= 0.4                                   # the drift-free class table (solve.hip: at most 0.5)
    shared = isinstance(names, str)
    levels = c.levels(names, True) if shared else [c.levels(n, True) for n in names]
    dev, ns = c.dev, c.ns
    for s in range(ns):
        dev.amg_clear(1 + s)
    if shared:
        dev.amg_upload(1, c.host.dg2cg, levels, ncol=ns)
    else:
        for s in range(ns):
            dev.amg_upload(1 + s, c.host.dg2cg, levels[s])
    b2 = c.b_knp.copy()
    b2[1] *= 1.0 + 1e-3 * np.random.default_rng(17).uniform(-1.0, 1.0, size=b2[1].shape)
    try:
        got = {k: (c.knp(k, c.b_knp), c.knp(k, c.b_knp), c.knp(k, b2, keep_bound=True) if independent and ns > 1 else None) for k in (1, 2)}
    finally:
        for s in range(ns):
            dev.amg_clear(1 + s)
        dev.upload(c.A.F_B_KNP, c.b_knp)
        dev.upload(c.A.F_C, c.host.pb.c)
    bad = []
    for k, (x, again, other) in got.items():
        assert np.array_equal(x, again), (names, k, "a second identical solve gave other bits")
        if other is not None:
            keep = [s for s in range(ns) if s != 1]
            assert np.array_equal(other[keep], x[keep]) and not np.array_equal(other[1], x[1]), (names, k, "species are not independent")
        x64 = ar.knp_xk(c.host, levels, k, bs=c.b_knp, blocks=blocks)
        xhp = ar.knp_xk(c.host, levels, k, ar.hp_dtype(), bs=c.b_knp, blocks=blocks)
        for s in range(ns):
            bd, err = ar.bound(x64[s], xhp[s]), np.abs(x[s] - x64[s]).max()
            _report("knp %s%s%s ns=%d %s species %d" % ("" if blocks == "cell" else "table ", c.host.mesh_name,
                                                        " 4 materials" if c.host.materials else "", ns, names, s), k, bd, err,
                    np.abs(xhp[s]).max())
            if not err <= bd:
                bad.append((k, s, err / bd))
    assert not bad, (names, bad)


@pytest.mark.parametrize("name", ALL)
def test_knp_iterates_two_species_shared(hip_lib, name):
    """two interleaved columns: the NC = 2 kernels"""
    _check_knp(_ctx("box_P1"), name)


@pytest.mark.parametrize("ns,name", [(3, "bands"), (3, "coarse_257"), (4, "bands"), (4, "coarse_1030")])
def test_knp_iterates_more_species_shared(hip_lib, ns, name):
    """three columns (NC = 1, grid.y = 3) and four (NC = 2, two column groups)"""
    _check_knp(_ctx("box_P1", IONS[ns]), name)


@pytest.mark.parametrize("ns,name", [(2, "bands"), (2, "coarse_769"), (3, "bands_t0")])
def test_knp_iterates_p2(hip_lib, ns, name):
    _check_knp(_ctx("box_P2", IONS[ns]), name)


@pytest.mark.parametrize("mesh,ns,names", [("box_P1", 2, ("bands", "mid")), ("box_P1", 3, ("bands", "bands_t0", "coarse_2")),
                                           ("box_P2", 2, ("bands_t0", "coarse_33"))])
def test_knp_iterates_one_hierarchy_per_species(hip_lib, mesh, ns, names):
    """different hierarchies in the species' slots (a mix-up shows); their V-cycles run on forked streams"""
    _check_knp(_ctx(mesh, IONS[ns]), names)


def test_knp_iterates_unfused_restriction(hip_lib, monkeypatch):
    monkeypatch.setenv("KNP_FUSE_RESTRICT", "0")
    _check_knp(_ctx("box_P1"), "bands", independent=False)


# ---- the eager V-cycle -------------------------------------------------------------------------------------------------------------
def _eager_cases(c):
    """x_k of: EMI with `bands` and `bands_t0`, both DG smoothers, k = 1, 2, 3; KNP with `bands` shared by the two species, k = 1, 2 --
    uploads and solves in the order of _check_emi / _check_knp.  Run by the test below (graph replay) and by its child process
    tests/amg_eager_worker.py (KNP_NO_GRAPH=1)."""
    dev, out = c.dev, {}
    for name in ("bands", "bands_t0"):
        for cheb in (False, True):
            dev.emi_residual_target(0.0)
            dev.amg_upload(0, c.host.dg2cg, c.levels(name))
            dev.set_emi_dg_smoother(cheb)
            try:
                for k in (1, 2, 3):
                    out["emi %s %d %d" % (name, cheb, k)] = c.emi(k, c.b_emi)
            finally:
                dev.set_emi_dg_smoother(None)
                dev.amg_clear(0)
                dev.upload(c.A.F_B_EMI, c.b_emi)
    for s in range(c.ns):
        dev.amg_clear(1 + s)
    dev.amg_upload(1, c.host.dg2cg, c.levels("bands", True), ncol=c.ns)
    try:
        for k in (1, 2):
            out["knp bands %d" % k] = c.knp(k, c.b_knp)
    finally:
        for s in range(c.ns):
            dev.amg_clear(1 + s)
        dev.upload(c.A.F_B_KNP, c.b_knp)
        dev.upload(c.A.F_C, c.host.pb.c)
    return out


def test_eager_vcycle_matches_the_replica_and_the_graph_replay(hip_lib, tmp_path, monkeypatch, capfd):
    """KNP_NO_GRAPH is read once per process, and the eager V-cycle is what runs whenever graph capture fails: one fresh child process
    with KNP_NO_GRAPH=1 runs _eager_cases on box_P1 (it reports no capture).  Its iterates must lie within the replica's bound, exactly
    as in _check_emi / _check_knp, and have the bits of this process's graph-replay run of the same cases: the same kernels in the
    same order on the same data.  That this process did replay is asserted too: with KNP_DEBUG the library reports every capture, one per
    uploaded hierarchy (four EMI uploads and the shared KNP one), each with an instantiated graph."""
    import os
    import subprocess
    import sys
    c = _ctx("box_P1")
    assert c.ns == 2
    out = str(tmp_path / "eager.npz")
    env = dict(os.environ, KNP_NO_GRAPH="1", KNP_DEBUG="1")
    run = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "amg_eager_worker.py"), out], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-3000:]
    assert "graph capture" not in run.stdout and "BeginCapture" not in run.stdout, "the child captured a graph"
    eager = dict(np.load(out))
    monkeypatch.setenv("KNP_DEBUG", "1")                              # (read at every capture)
    capfd.readouterr()
    replay = _eager_cases(c)
    captures = [l for l in capfd.readouterr().err.splitlines() if "V-cycle graph capture" in l]
    monkeypatch.delenv("KNP_DEBUG")
    assert len(captures) == 5 and all("rc=0 end=0 exec=0x" in l for l in captures), captures
    assert sorted(eager) == sorted(replay) and len(eager) == 14
    bad, other_bits = [], []
    for key, x in eager.items():
        system, name, *rest = key.split()
        k = int(rest[-1])
        if system == "emi":
            cheb = bool(int(rest[0]))
            x64 = ar.emi_xk(c.host, c.levels(name), cheb, k, b=c.b_emi)[None]
            xhp = ar.emi_xk(c.host, c.levels(name), cheb, k, ar.hp_dtype(), b=c.b_emi)[None]
        else:
            x64 = ar.knp_xk(c.host, c.levels(name, True), k, bs=c.b_knp, blocks="cell")
            xhp = ar.knp_xk(c.host, c.levels(name, True), k, ar.hp_dtype(), bs=c.b_knp, blocks="cell")
        for s in range(len(x64)):
            bd, err = ar.bound(x64[s], xhp[s]), np.abs(np.atleast_2d(x)[s] - x64[s]).max()
            _report("eager %s species %d" % (key, s), k, bd, err, np.abs(xhp[s]).max())
            if not err <= bd:
                bad.append((key, s, err / bd))
        if not np.array_equal(x, replay[key]):
            other_bits.append((key, float(np.abs(x - replay[key]).max())))
    assert not bad, bad
    assert not other_bits, ("eager and replayed V-cycles gave other bits", other_bits)


# ---- KNP on the drift-free class table (solve.hip: build_bj_table) -----------------------------------------------------------------
def _check_knp_table(c, names, independent=True):
    """_check_knp at a potential whose cell Peclet number is below the switch: the device preconditions with its table, the replica
    with the oracle's drift-free blocks (amg_ref.Host.knp_table_blocks)"""
    _check_knp(c, names, independent, blocks="table")


def _table_ctx(mesh="box_P1", ns=2, materials=False):
    return _ctx(mesh, IONS[ns], ar.TABLE_PHI_SCALE, materials)


@pytest.mark.parametrize("case", ar.TABLE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_knp_table_iterates(hip_lib, case):
    """every key's block (24 geometry classes, 42 keys; 100 / 72 with four materials), bj_idx in device cell order, all the Krylov vector
    kernels that read through bj_block() and the power iteration of the spectral bound"""
    mesh, ns, names, materials = case
    _check_knp_table(_table_ctx(mesh, ns, materials), names)


def test_knp_table_iterates_unfused_restriction(hip_lib, monkeypatch):
    monkeypatch.setenv("KNP_FUSE_RESTRICT", "0")
    _check_knp_table(_table_ctx(), "bands", independent=False)


# ---- the switch between the two block sets and its state ---------------------------------------------------------------------------
def _set_phi(c, phi, upload=True):
    """upload: a state upload (it resets the lagged state and last_peclet: the next solve reads the Peclet number itself).  Otherwise
    the potential changes on the device, as a time step changes it: through a same-sized field whose upload has no side effects."""
    A, dev = c.A, c.dev
    if upload:
        dev.upload(A.F_PHI, phi)
    else:
        dev.upload(A.F_B_EMI, phi)
        dev.copy_field(A.F_PHI, A.F_B_EMI)
    dev.update_dnphi()


@contextlib.contextmanager
def _bands(c):
    """the hierarchy `bands` shared by the species, for solves at other potentials / coefficients; the context's state afterwards"""
    dev, ns, A = c.dev, c.ns, c.A
    levels = c.levels("bands", True)
    for s in range(ns):
        dev.amg_clear(1 + s)
    dev.amg_upload(1, c.host.dg2cg, levels, ncol=ns)
    try:
        yield levels
    finally:
        for s in range(ns):
            dev.amg_clear(1 + s)
        set_params_of(dev, c.host.pb)
        dev.upload(A.F_B_KNP, c.b_knp)
        dev.upload(A.F_B_EMI, c.b_emi)
        dev.upload(A.F_C, c.host.pb.c)
        _set_phi(c, c.host.pb.phi)


def _match(c, host, levels, k, x, tag, blocks, lmax=None):
    """the device's x_k against the replica on `host`'s matrices with `blocks` (and the spectral bound `lmax`, default: estimated on
    these matrices and blocks from the right-hand side)"""
    x64 = ar.knp_xk(host, levels, k, bs=c.b_knp, blocks=blocks, lmax=lmax)
    xhp = ar.knp_xk(host, levels, k, ar.hp_dtype(), bs=c.b_knp, blocks=blocks, lmax=lmax)
    bad = []
    for s in range(c.ns):
        bd, err = ar.bound(x64[s], xhp[s]), np.abs(x[s] - x64[s]).max()
        _report("knp switch %s %s species %d" % (c.host.mesh_name, tag, s), k, bd, err, np.abs(xhp[s]).max())
        if not err <= bd:
            bad.append((k, s, err / bd))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("pe,blocks", [(0.45, "table"), (0.55, "cell")])
def test_knp_switch_threshold(hip_lib, pe, blocks):
    """on either side of KNP_BJ_TABLE_PECLET = 0.5 (the float the device compares is 0.45 / 0.55 to 1e-7)"""
    c = _table_ctx()
    h = ar.at_peclet(c.host, pe)
    with _bands(c) as levels:
        _set_phi(c, h.pb.phi)
        for k in (1, 2):
            _match(c, h, levels, k, c.knp(k, c.b_knp), "Pe %.2f" % pe, blocks)


@pytest.mark.parametrize("mesh,pos", [("box_P1", p) for p in (0, 63, 64, 255, 256, -1)] + [("box_P2", -1)])
def test_knp_switch_finds_the_largest_cell_peclet_number(hip_lib, mesh, pos):
    """k_cell_peclet: one cell with Peclet number 0.8 in a background of 0.054, first and last lane of a wave, of a workgroup (256
    cells), of the grid (768 cells: three full workgroups; 324 on the P2 box: the second one partly filled) -- the solve must fall
    back to the per-cell blocks wherever the cell sits"""
    c = _table_ctx(mesh)
    h = ar.one_cell_peclet(c.host, int(c.dev.cell_order[pos if pos >= 0 else c.dev.nc_owned - 1]))
    with _bands(c) as levels:
        _set_phi(c, h.pb.phi)
        _match(c, h, levels, 1, c.knp(1, c.b_knp), "cell %d of the device" % pos, "cell")


def test_knp_switch_falls_back_and_returns_without_an_upload(hip_lib):
    """amg_ref.switch_sequence (the rules of solve.hip are written there): the potential changes on the device, through a field whose
    upload has no side effects, and x_0 = 0 likewise (Ctx.knp(keep_bound=True)); every solve is one BiCGStab iteration.  That each
    step tells its rule from a broken one by >= 1e6 bounds is asserted on the CPU (tests/test_amg_ref_host.py)."""
    c = _table_ctx()
    assert abs(c.host.peclet() - 0.27) < 0.005
    with _bands(c) as levels:
        last = None
        for i, st in enumerate(ar.switch_sequence(c.host, c.b_knp)):
            if st["phi"] is not None:
                _set_phi(c, st["phi"].pb.phi, upload=i == 0)
            x = c.knp(1, c.b_knp, keep_bound=i > 0)                     # (the first one: upload of c, x_0 = 0 and an empty history)
            _match(c, st["host"], levels, 1, x, st["tag"], st["blocks"], st["lmax"])
            if st["tag"] == "6 low again":
                assert np.array_equal(x, last), "a table solve with the kept bound gave other bits"
            last = x


@pytest.mark.parametrize("what", ["dt", "materials"])
def test_knp_table_is_rebuilt_after_new_coefficients(hip_lib, what):
    """set_params with half the time step, or with the four-material diffusion coefficients, on a context whose table exists: the
    next solve runs on the table of the new coefficients (same mesh, same state)"""
    c = _table_ctx()
    h = c.host.variant(dt=c.host.pb.dt / 2) if what == "dt" else c.host.variant(D=ar.four_materials(c.host.pb))
    with _bands(c) as levels:
        _match(c, c.host, levels, 1, c.knp(1, c.b_knp), "before new %s" % what, "table")
        set_params_of(c.dev, h.pb)
        c.dev.update_dnphi()
        _match(c, h, levels, 1, c.knp(1, c.b_knp), "new %s" % what, "table")


# ---- restarted GMRES, iterate by iterate (krylov.hip: gmres_impl; krylov_scalar.hpp: gm_scalar_op) ---------------------------------
@contextlib.contextmanager
def _gmres_on(c, names, m):
    """the hierarchies `names` in the KNP slots and GMRES(m) as the KNP method; afterwards BiCGStab and the context's state again
    (contexts are shared by the tests of this module)"""
    shared = isinstance(names, str)
    levels = c.levels(names, True) if shared else [c.levels(n, True) for n in names]
    dev, ns = c.dev, c.ns
    for s in range(ns):
        dev.amg_clear(1 + s)
    if shared:
        dev.amg_upload(1, c.host.dg2cg, levels, ncol=ns)
    else:
        for s in range(ns):
            dev.amg_upload(1 + s, c.host.dg2cg, levels[s])
    dev.set_knp_krylov("gmres", m)
    try:
        yield levels
    finally:
        dev.set_knp_krylov("bicgstab")
        for s in range(ns):
            dev.amg_clear(1 + s)
        dev.upload(c.A.F_B_KNP, c.b_knp)
        dev.upload(c.A.F_C, c.host.pb.c)


def _assert_block_set(c, blocks):
    if blocks == "cell":
        assert c.host.peclet() > 0.5
    else:
        assert c.host.peclet() <= 0.4


@pytest.mark.parametrize("case", ar.GM_CASES, ids=lambda c: "-".join(str(v) for v in c[:5]))
def test_gmres_iterates(hip_lib, case):
    """x_k of GMRES(m) for every count of the case (amg_ref.GM_CASES: what the counts reach is written and asserted there) against
    amg_ref.gmres, within the bound of the three replica runs; each solve twice with the same bits; and with another right-hand side
    for species 1 the other species keep their bits (the spectral bound held fixed, as in _check_knp)."""
    mesh, ns, names, blocks, m, ks = case
    c = _ctx(*ar.gm_host_args(case))
    assert c.ns == ns
    _assert_block_set(c, blocks)
    b2 = c.b_knp.copy()
    b2[1] *= 1.0 + 1e-3 * np.random.default_rng(17).uniform(-1.0, 1.0, size=b2[1].shape)
    with _gmres_on(c, names, m) as levels:
        got = {k: (c.knp(k, c.b_knp), c.knp(k, c.b_knp), c.knp(k, b2, keep_bound=True)) for k in ks}
    ref = ar.gm_reference(c.host, levels, blocks, m, ks, bs=c.b_knp)
    bad = []
    keep = [s for s in range(ns) if s != 1]
    for k, (x, again, other) in got.items():
        assert np.array_equal(x, again), (case, k, "a second identical solve gave other bits")
        assert np.array_equal(other[keep], x[keep]) and not np.array_equal(other[1], x[1]), (case, k, "species are not independent")
        x64, bds, scales = ref[k]
        for s in range(ns):
            err = np.abs(x[s] - x64[s]).max()
            _report("gmres(%d) %s%s ns=%d %s species %d" % (m, "" if blocks == "cell" else "table ", mesh, ns, names, s), k, bds[s], err,
                    scales[s])
            if not err <= bds[s]:
                bad.append((k, s, err / bds[s]))
    assert not bad, (case, bad)


@pytest.mark.parametrize("case", ar.GM_FREE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_gmres_converged_solves_follow_the_replica(hip_lib, case):
    """the solve run to convergence (min_it = 0, a look after every iteration) on the cases whose decisions tests/test_amg_ref_host.py
    shows >= 1e-3 away from their thresholds: per species the iteration count of amg_ref.gmres_free (cycle ends on KS_GM_T2, idling
    until every species' cycle is done, the joint restart, the test on the true residual), the iterate within the bound, and the
    reported residual norm res[:, 1] within 1e-6 of the host's norm of b - A x for the returned x."""
    name, rtol, m = case
    c = _table_ctx()
    _assert_block_set(c, "table")
    A, dev = c.A, c.dev
    mats = c.host.knp()[0]
    with _gmres_on(c, name, m) as levels:
        dev.upload(A.F_B_KNP, c.b_knp)
        dev.upload(A.F_C, np.zeros(c.ns * c.host.pb.ndof))
        niter, res = dev.knp_solve(rtol, maxit=400, min_it=0, check_every=1)
        x = dev.download(A.F_C).reshape(c.ns, -1)
    runs, bds, scales, margin = ar.gm_free_reference(c.host, levels, rtol, m, bs=c.b_knp)
    assert margin >= 1e-3, margin
    bad = []
    for s in range(c.ns):
        err = np.abs(x[s] - runs[s]["x"]).max()
        true = c.host.ref.norm_d8(c.b_knp[s] - mats[s] @ x[s])
        print("AMGPAR gmres(%d) free %s rtol %g species %d: niter %d (replica %d, cycles %s) bound %.2e err %.2e res %.6e host %.6e"
              % (m, name, rtol, s, niter[s], runs[s]["niter"], runs[s]["cycles"], bds[s] / scales[s], err / scales[s], res[s, 1], true))
        if niter[s] != runs[s]["niter"]:
            bad.append((s, "niter", niter[s], runs[s]["niter"]))
        elif not err <= bds[s]:
            bad.append((s, "iterate", err / bds[s]))
        if not abs(res[s, 1] / true - 1.0) <= 1e-6:
            bad.append((s, "res", res[s, 1], true))
    assert not bad, (case, bad)
