"""CPU side of the head / tail cases of tests/apply_split_cases.py: every case has the property it exists for (so that a mesh or
seed change cannot quietly empty it), stated through `block_stats` -- the restatement of both table builders that
tests/test_gpu_tables.py compares with the device's tables entry for entry -- and the meshes of the older partition and
unstructured tests have NO overflowing block: before these cases the head of every apply the suite ran covered all owned cells."""
import numpy as np
import pytest

import apply_split_cases as ac
from knpemidg import _abi

_MESH = {}


def _base(kind):
    if kind not in _MESH:
        _MESH[kind] = ac.base_mesh(kind)
    return _MESH[kind]


def _stats(kind, name):
    m, s, f = _base(kind)
    order = ac.case_order(name, m)
    return m, order, ac.block_stats(m, order, m.num_cells(), f.array(), (1,))


def test_device_cell_order_is_the_order_of_a_context():
    """device_cell_order is what Device numbers its cells by (the function Device.__init__ calls): a Morton curve over the owned cells'
    midpoints scaled by the median cell extent, interior cells of a partition first; the caller's order without reordering."""
    m, s, f = _base("S")
    nc = m.num_cells()
    order, n_int = _abi.device_cell_order(m, nc, True)
    xc = m.coords[m.cells]
    scale = np.maximum(np.median(xc.max(axis=1) - xc.min(axis=1), axis=0), 1e-300)
    assert n_int == nc and np.array_equal(order, _abi.morton_order(m.cell_midpoints(), scale))
    o2, n2 = _abi.device_cell_order(m, nc, False)
    assert n2 == nc and np.array_equal(o2, np.arange(nc))
    loc, sub_l, surf_l = ac.partition_rank((6, 10, 10), "S", 0)[:3]
    no = loc.nc_owned
    order, n_int = _abi.device_cell_order(loc.mesh, no, True)
    assert np.array_equal(np.sort(order[:no]), np.arange(no)) and np.array_equal(order[no:], np.arange(no, loc.mesh.num_cells()))
    fc = loc.mesh.facet_cells
    both = fc[:, 1] >= 0
    touches_ghost = np.zeros(loc.mesh.num_cells(), dtype=bool)
    cut = both & ((fc[:, 0] >= no) != (fc[:, 1] >= no))
    touches_ghost[fc[cut].ravel()] = True
    assert n_int == 1600 and not touches_ghost[order[:n_int]].any() and touches_ghost[order[n_int:no]].all()


def test_permuted_mesh_carries_cells_and_tags():
    m, s, f = _base("J")
    perm = np.random.default_rng(0).permutation(m.num_cells())
    pm, ps, pf = ac.permuted_mesh(m, s, f, perm)
    assert np.array_equal(pm.cells, m.cells[perm]) and np.array_equal(ps.array(), s.array()[perm]) and pm.coords is not m.coords
    old = {tuple(v): int(t) for v, t in zip(m.facets.tolist(), f.array().tolist())}
    assert [old[tuple(v)] for v in pm.facets.tolist()] == pf.array().tolist()
    assert np.bincount(pf.array()).tolist() == np.bincount(f.array()).tolist() and (pf.array() == 1).sum() > 0
    # the same coupling whether stated with the tags or without: every interior facet of these boxes is SIPG or membrane
    o = np.arange(m.num_cells())
    a, b = ac.block_stats(pm, o, len(o)), ac.block_stats(pm, o, len(o), pf.array(), (1,))
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kind,name", sorted(ac.EXPECT))
def test_case_has_its_property(kind, name):
    m, order, st = _stats(kind, name)
    nblk = 14
    assert m.num_cells() == 3456 and len(st["lists_s"]) == nblk and np.array_equal(np.sort(order), np.arange(3456))
    exp = ac.EXPECT[(kind, name)][0]
    got_s, got_u = ac.expected_structured(st), ac.expected_unstructured(st)
    assert (got_s if kind == "S" else got_u) == exp
    ls, lu, v = st["lists_s"], st["lists_u"], st["verts"]
    assert np.array_equal(ls, lu)                                  # one context owns every cell: the two list rules agree
    fits_u = (lu <= ac.LIST_U) & (v <= ac.VERT_U)
    if name == "A":                                                # the Morton order itself: far below every limit
        assert ls.max() == 168 and v.max() == 185 and got_s[0] == got_u[0] == nblk
    elif name in ("B1", "B7"):                                     # both builders stop at block k; everything behind it is far over
        k = int(name[1:])
        assert got_s[0] == got_u[0] == k and ls[k:-1].min() > 750 and v[k:-1].min() > 400 and ls[:k].max() <= 168
    elif name == "C":                                              # two blocks over one entry per thread, under the 320 of the unstructured ring
        assert got_s[0] == 5 and got_u[0] == nblk and fits_u.all()
        assert sorted(np.nonzero(lu > 256)[0].tolist()) == [5, 6] and ls[[5, 6]].tolist() == ([307, 305] if kind == "S" else [298, 292])
    elif name in ("D1", "D6"):                                     # over 320: the unstructured ring stops in front of the pair
        k = int(name[1:])
        assert got_u[0] == k and lu[k] > ac.LIST_U and lu[k + 1] > 256 and v[[k, k + 1]].max() <= ac.VERT_U and fits_u[:k].all()
    elif name == "E_lists":                                        # exactly 320 entries stay in the head, 321 start the tail
        assert lu[3] == 320 and lu[8] == 321 and fits_u[:8].all() and v.max() <= ac.VERT_U and got_u == (8, 320)
    elif name == "E_verts":                                        # exactly 256 vertices (byte position 255) stay, 257 do not
        assert v[3] == 256 and v[8] == 257 and fits_u[:8].all() and lu.max() <= ac.LIST_U and got_u[0] == 8
    elif name == "E_struct":                                       # exactly one entry per thread stays, 257 do not
        assert ls[3] == 256 and ls[8] == 257 and ls[:8].max() == 256 and got_s == (8, 256)
    elif name == "F":                                              # everything fits, the longest list is beyond the ring's 224
        assert got_s[0] == nblk and ac.RING_S < ls.max() == 240 <= ac.LIST_S
    elif name == "G":                                              # the first block already overflows both
        assert ls[0] > ac.LIST_U and v[0] > ac.VERT_U and got_s == got_u == (0, 0)
    else:
        raise KeyError(name)


@pytest.mark.parametrize("box,kind", sorted(ac.PARTITIONS))
def test_partition_has_its_property(box, kind):
    for rank in (0, 1):
        loc, sub_l, surf_l = ac.partition_rank(box, kind, rank)[:3]
        no = loc.nc_owned
        order, n_int = _abi.device_cell_order(loc.mesh, no, True)
        st = ac.block_stats(loc.mesh, order, no, surf_l.array(), (1,))
        s, u = ac.expected_structured(st), ac.expected_unstructured(st)
        nblk = len(st["lists_s"])
        if box == (6, 10, 10):
            # the cells on the cut sit in a plane at the end of the order: their block overflows everything
            assert no == 1800 and nblk == 8 and n_int == 1600 and s[0] == u[0] == 6 and n_int > s[0] * ac.B
            assert st["lists_s"][6] > 600 and st["verts"][6] > ac.VERT_U and s[1] <= ac.RING_S
        elif box == (6, 8, 8):
            assert no == 1152 and nblk == 5 and n_int == 1024 and s == (5, 240) and st["lists_s"][4] == 240
        else:
            # all three blocks fit; the ghosts numbered 576.. fall into the id range of the last block [512, 768) and are not in it
            assert no == 576 and nblk == 3 and u[0] == 3 and 0 < n_int < no
            assert st["lists_u"][2] > st["lists_s"][2] and np.array_equal(st["lists_u"][:2], st["lists_s"][:2])


def _no_overflow(mesh, n_own, ftags, mtags):
    order = _abi.device_cell_order(mesh, n_own, True)[0]
    st = ac.block_stats(mesh, order, n_own, ftags, mtags)
    nblk = len(st["lists_s"])
    return ac.expected_structured(st)[0] == nblk, ac.expected_unstructured(st)[0] == nblk


def test_older_partition_and_unstructured_meshes_never_overflow_a_block():
    """test_partitioned_kernels_on_one_gpu (structured kernels, (12, 4, 4) in 2 slabs and 3 RCB parts) and
    test_unstructured_apply_kernel_variants (variant 10: tissue piece, its refinement, jittered box): the head covers every owned cell."""
    from knpemidg.partition import Partition
    from common import small_3d
    m, s, f = small_3d((12, 4, 4))
    for world, method in ((2, "slab"), (3, "rcb")):
        part = Partition(m, world, method=method)
        for rank in range(world):
            loc = part.local(rank)
            surf_l = loc.localize(s, f, (1,))[1]
            assert _no_overflow(loc.mesh, loc.nc_owned, surf_l.array(), (1,))[0]
    import emix_sub
    from knpemidg.mesh import refine_uniform
    m, s, f = emix_sub.emix_submesh()
    assert _no_overflow(m, m.num_cells(), f.array(), (1, 2))[1]
    assert _no_overflow(refine_uniform(m)[0], 8 * m.num_cells(), None, ())[1]      # (its membrane tags only drop couplings: untagged is the upper bound)
    m, s, f = _base("J")
    assert _no_overflow(m, m.num_cells(), f.array(), (1,))[1]
