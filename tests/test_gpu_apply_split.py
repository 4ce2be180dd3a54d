"""Operator applies whose staged HEAD kernel stops short of the mesh (csrc/apply_plan.hpp: head = ring- / halo-staged persistent
kernel on the leading blocks that fit its staging limits, tail = thread-per-cell kernel on the rest) against the oracle's assembled
operators (reference: src/knpemidg/solver.py:325-328, 346 for a_emi; :586-594 for A_knp) at the tolerance of test_gpu_parity.py.

The cases are the seeded cell orders of tests/apply_split_cases.py (their properties are asserted on the CPU by
tests/test_apply_split_host.py); the device gets the permuted mesh with KNP_NO_REORDER=1, so the caller's order is the device order.
Every test asserts the apply variant and how many cells the head covers (KNP_DT_META on the structured mesh S, KNP_DT_RU_META on
the jittered mesh J), so a case cannot silently run another kernel than the one it is about.  The result vector is filled with NaN
before every apply: a row that no launch writes fails the comparison.

Range cuts: with KNP_FORCE_SPLIT=1 an apply is an interior launch [0, n) and a boundary launch [n, nc_owned) (csrc/comm.hip:
dist_apply), each of them head and / or tail.  Every row is produced by the same kernel from the same inputs whichever launch
carries it, so the split results equal the one-launch result of the same context BIT FOR BIT."""
import numpy as np
import pytest

import apply_split_cases as ac
import knpemi_oracle as ko
from common import synthetic_state, device_for, push_state, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-11                  # test_gpu_parity.py: pure re-orderings of the same floating-point sums
_MESH, _REF = {}, {}


def _problem(kind, name, one_species=False):
    """(problem on the permuted mesh, seeded x, oracle A_emi x [nc, 4], oracle A_knp,k x_k [ns, nc, 4]): computed once per case"""
    key = (kind, name, one_species)
    if key not in _REF:
        if kind not in _MESH:
            _MESH[kind] = ac.base_mesh(kind)
        m, s, f = _MESH[kind]
        pm, ps, pf = ac.permuted_mesh(m, s, f, ac.case_order(name, m))
        if one_species:
            # two ions, one solved: K and the eliminated Na, D per subdomain (two materials)
            P = ko.idealized_params()
            tags = ps.array().astype(np.int64)
            ions = [dict(name=n, z=P["z"][n], D=P["D"][n] * np.array([1.0, 0.5])[np.minimum(tags, 1)]) for n in ("K", "Na")]
            pb = ko.Problem(pm, tags, pf.array(), 1, ions, P, membrane_tags=(1,))
            rng = np.random.default_rng(17)
            pb.c = rng.uniform(50.0, 150.0, size=pb.c.shape)
            pb.c_prev_n = pb.c.copy()
            pb.c_elim = rng.uniform(50.0, 150.0, size=pb.c_elim.shape)
        else:
            pb = ko.build_idealized(pm, ps.array(), pf.array(), membrane_tags=(1,))
        x = synthetic_state(pb)
        ye = (ko.assemble_emi(pb, want_B=False)[0] @ x[0].ravel()).reshape(-1, 4)
        yk = np.stack([(ko.assemble_knp(pb, k) @ x[k].ravel()).reshape(-1, 4) for k in range(pb.N_ions)])
        for a in (x, ye, yk):
            a.setflags(write=False)
        _REF[key] = (pb, x, ye, yk)
    return _REF[key]


def _device(pb, monkeypatch, **kw):
    from knpemidg import _abi as A
    monkeypatch.setenv("KNP_NO_REORDER", "1")
    dev = device_for(pb, **kw)
    assert np.array_equal(dev.cell_order, np.arange(dev.nc))
    push_state(dev, pb)
    dev.update_kappa(); dev.update_dnphi()
    return dev, A


def _applies(dev, A, x, rows=None):
    """(A_emi x, A_knp x) of the context, owned rows, from a result vector that held NaN"""
    rows = dev.nc_owned if rows is None else rows
    ns = x.shape[0]
    nan = np.full(dev.size(A.F_Y), np.nan)
    dev.upload(A.F_Y, nan)
    dev.upload(A.F_X, x[0]); dev.emi_apply(A.F_X, A.F_Y)
    ye = dev.download(A.F_Y, 0, dev.nc * 4).reshape(-1, 4)[:rows].copy()
    dev.upload(A.F_Y, nan)
    dev.upload(A.F_X, x); dev.knp_apply(A.F_X, A.F_Y)
    yk = dev.download(A.F_Y).reshape(ns, -1, 4)[:, :rows].copy()
    return ye, yk


def _coverage(dev, A, kind, key):
    """asserts variants and table sizes of case `key`; returns head_cells of (EMI, KNP) -- nc_owned where no staged head runs"""
    (long0, hs), variants = ac.EXPECT[key]
    assert (dev.apply_variant(0), dev.apply_variant(1)) == variants
    meta, ru = dev.debug_table(A.DT_META), dev.debug_table(A.DT_RU_META)
    no = dev.nc_owned
    if kind == "S":
        assert dev.n_geometry_classes > 0 and (int(meta[5]), int(meta[4])) == (long0, hs)
        assert ru.size == 0 and all(dev.debug_table(t).size == 0 for t in range(A.DT_RU_HB_SRC, A.DT_RU_HINV4 + 1))
        head = min(long0 * ac.B, no)
        return tuple(head if v in (2, 3, 6, 7) else no for v in variants)
    assert dev.n_geometry_classes == 0
    if long0 == 0:
        assert ru.size == 0 and all(dev.debug_table(t).size == 0 for t in range(A.DT_RU_HB_SRC, A.DT_RU_HINV4 + 1))
        return no, no
    nblk = (no + ac.B - 1) // ac.B
    assert ru.tolist() == [long0, hs, nblk, min(long0 * ac.B, no)]
    return int(ru[3]), int(ru[3])


def _check(ye, yk, pb, ref_e, ref_k):
    assert relerr(ye, ref_e) < TOL
    for k in range(pb.N_ions):
        assert relerr(yk[k], ref_k[k]) < TOL


@pytest.mark.parametrize("kind,name", sorted(ac.EXPECT))
def test_head_and_tail_applies_vs_oracle(hip_lib, monkeypatch, kind, name):
    """One launch over all cells = head + tail.  Numbers the device confirmed (blocks covered, stride / longest list):
    S: A 14, 168 (variants 3 / 7); B1 1, 88; B7 7, 168; C 5, 168; E_struct 8, 256 (1 / 6: the ring refuses a 256-entry stride); F 14, 240
    (1 / 6); G none (1 / 1).  J (variant 10): A 14, 168; B1 1, 86; B7 7, 168; C 14, 298; D1 1, 86; D6 6, 168; E_lists 8, 320; E_verts 8, 207;
    G none (0 / 0)."""
    pb, x, ref_e, ref_k = _problem(kind, name)
    dev, A = _device(pb, monkeypatch)
    try:
        _coverage(dev, A, kind, (kind, name))
        _check(*_applies(dev, A, x), pb, ref_e, ref_k)
    finally:
        dev.close()


def test_halo_kernel_with_per_cell_coefficients_on_a_list_beyond_the_ring(hip_lib, monkeypatch):
    """Case F without the material table: the halo-staged kernel that reads D per cell (variant 2) on a 240-entry stride."""
    pb, x, ref_e, ref_k = _problem("S", "F")
    monkeypatch.setenv("KNP_APPLY_MAT", "0")
    dev, A = _device(pb, monkeypatch)
    try:
        assert (dev.apply_variant(0), dev.apply_variant(1)) == (1, 2)
        _check(*_applies(dev, A, x), pb, ref_e, ref_k)
    finally:
        dev.close()


@pytest.mark.parametrize("kind,name", [(k, n) for k in "SJ" for n in ("B7", "C")])
def test_one_solved_species_vs_oracle(hip_lib, monkeypatch, kind, name):
    """The NS = 1 instances of the ring-staged KNP kernels (variants 7 and 10) with a head that stops inside the mesh, D from a
    two-material table."""
    pb, x, ref_e, ref_k = _problem(kind, name, one_species=True)
    assert pb.N_ions == 1
    dev, A = _device(pb, monkeypatch)
    try:
        _coverage(dev, A, kind, (kind, name))
        _check(*_applies(dev, A, x), pb, ref_e, ref_k)
    finally:
        dev.close()


def _range_cuts(dev, A, monkeypatch, pb, x, ref_e, ref_k, cuts, rows=None):
    monkeypatch.setenv("KNP_FORCE_SPLIT", "0")
    ye1, yk1 = _applies(dev, A, x, rows)
    _check(ye1, yk1, pb, ref_e, ref_k)
    monkeypatch.setenv("KNP_FORCE_SPLIT", "1")
    for n in cuts:
        dev.set_interior(n)
        assert int(dev.debug_table(A.DT_META)[6]) == n
        ye, yk = _applies(dev, A, x, rows)
        _check(ye, yk, pb, ref_e, ref_k)
        assert np.array_equal(ye, ye1) and np.array_equal(yk, yk1), "cut at %d: not the one-launch result bit for bit" % n


@pytest.mark.parametrize("kind,name", [(k, n) for k in "SJ" for n in ("B1", "B7", "C")])
def test_range_cuts_around_the_head_boundary(hip_lib, monkeypatch, kind, name):
    """Interior + boundary launches with the cut at both ends, around a block edge, inside the head, exactly on head_cells, one cell
    either side of it and inside the tail: each against the oracle and bit for bit against the one-launch result."""
    pb, x, ref_e, ref_k = _problem(kind, name)
    dev, A = _device(pb, monkeypatch)
    try:
        head = _coverage(dev, A, kind, (kind, name))[1]
        no = dev.nc_owned
        assert (head == no) == (name == "C" and kind == "J")      # C on J: the unstructured ring takes all blocks, cuts fall inside the head only
        if name == "C" and kind == "J":
            head = 5 * ac.B                                        # ... so cut around the first block that uses the second list piece
        cuts = ac.cut_points(head, no)
        assert {1, 255, 256, 257, head - 1, head, head + 1, no - 1} <= set(cuts)
        _range_cuts(dev, A, monkeypatch, pb, x, ref_e, ref_k, cuts)
    finally:
        dev.close()


@pytest.mark.parametrize("box,kind", sorted(ac.PARTITIONS))
def test_partition_with_a_head_short_of_the_owned_cells(hip_lib, monkeypatch, box, kind):
    """Owned + ghost contexts of a box cut in two slabs, in the device's own order (Morton, interior cells first), ghosts filled from
    the global arrays as the halo exchange delivers them: the owned rows of the global oracle results, in one launch and as
    interior + boundary launches at the partition's own n_interior -- on (6, 10, 10) that one lies BEHIND head_cells, so the boundary
    launch runs the tail kernel alone -- and, on (6, 10, 10), at every cut the ghost rule of knp_set_interior admits."""
    from knpemidg import _abi as A
    m, s, f = ac.base_mesh(kind, box)
    pbg = ko.build_idealized(m, s.array(), f.array(), membrane_tags=(1,))
    x = synthetic_state(pbg)
    yg = (ko.assemble_emi(pbg, want_B=False)[0] @ x[0].ravel()).reshape(-1, 4)
    ykg = np.stack([(ko.assemble_knp(pbg, k) @ x[k].ravel()).reshape(-1, 4) for k in range(pbg.N_ions)])
    for rank in (0, 1):
        loc, sub_l, surf_l = ac.partition_rank(box, kind, rank)[:3]
        pbl = ko.build_idealized(loc.mesh, sub_l.array(), surf_l.array(), membrane_tags=(1,))
        cg, no = loc.cells_global, loc.nc_owned
        pbl.c, pbl.c_prev_n, pbl.c_elim, pbl.phi = pbg.c[:, cg], pbg.c_prev_n[:, cg], pbg.c_elim[cg], pbg.phi[cg]
        order, n_int = A.device_cell_order(loc.mesh, no, True)
        st = ac.block_stats(loc.mesh, order, no, surf_l.array(), (1,))
        dev = device_for(pbl, nc_owned=no)
        try:
            assert np.array_equal(dev.cell_order, order) and dev.n_interior == n_int
            push_state(dev, pbl)
            dev.update_kappa(); dev.update_dnphi()
            meta, ru = dev.debug_table(A.DT_META), dev.debug_table(A.DT_RU_META)
            nblk = (no + ac.B - 1) // ac.B
            variants = (dev.apply_variant(0), dev.apply_variant(1))
            if kind == "S":
                long0, hs = ac.expected_structured(st)
                assert (int(meta[5]), int(meta[4])) == (long0, hs) and ru.size == 0 and int(meta[6]) == n_int
                assert variants == ((3, 7) if box == (6, 10, 10) else (1, 6))
                head = long0 * ac.B
            else:
                long0, hs = ac.expected_unstructured(st)
                assert ru.tolist() == [long0, hs, nblk, min(long0 * ac.B, no)] and variants == (10, 10)
                head = int(ru[3])
            assert (head < n_int) == (box == (6, 10, 10)) and (long0 < nblk) == (box == (6, 10, 10))
            # the caller-order views of the device: row d of what _applies returns is the caller's local cell d
            ref_e, ref_k = yg[cg[:no]], ykg[:, cg[:no]]
            xl = np.ascontiguousarray(x[:, cg])
            cuts = [n_int]
            if box == (6, 10, 10):
                cuts = [n for n in ac.cut_points(head, no) if n <= n_int] + [n_int]
                assert {1, 255, 256, 257, head - 256, head - 1, head, head + 1, 1600} <= set(cuts)
            _range_cuts(dev, A, monkeypatch, pbl, xl, ref_e, ref_k, cuts, rows=no)
            # one cell more than the interior has a ghost neighbour: knp_set_interior refuses it
            with pytest.raises(A.KnpError):
                dev.set_interior(n_int + 1)
        finally:
            dev.close()
