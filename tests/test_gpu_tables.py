"""Bit-exact parity of the connectivity / orientation tables (`north_star`: "bit-exact for DoF/connectivity indexing").

The library derives its neighbour, flag (neighbour-local facet, integration class, plus-side bit), facet-id, membrane-facet and
halo-block tables inside `knp_ctx_create` (csrc/context.hip) from raw cells / tags -- the device counterpart of DOLFIN's facet
topology, of the `dS(tag)` classification (reference: src/knpemidg/solver.py:113-121) and of `interface_normal` / `plus` /
`minus` (reference: src/knpemidg/utils.py:61-98).  They are read back through `knp_debug_table` and compared ENTRY FOR ENTRY with
the tables `oracle/connectivity.py` derives independently (dictionary matching of sorted vertex tuples in the caller's numbering,
none of the product's facet tables).  Integer data: every comparison is `array_equal`."""
import os
import sys

import numpy as np
import pytest

import connectivity as oc
from knpemidg import _abi as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mesh(which):
    from knpemidg.mesh import make_mesh_2D, make_mesh_3D
    if which == "2D_r0":
        return make_mesh_2D(0) + ((1,),)
    if which == "3D_4axon_r0":
        return make_mesh_3D(0, n_axons=4) + ((1, 2, 3, 4),)
    sys.path.insert(0, os.path.join(ROOT, "examples", "emix_simulations"))
    from emix_common import load_mesh
    return load_mesh() + ((1, 2),)


def _expected_halo_tables(nbr_d, nloc_d, kind_d, nc_owned, B=256):
    """Layout contract of KNP_DT_HB_SRC / KNP_DT_HB_LOC (include/knpemi_hip.h), restated: per block of B consecutive device cells
    the coupled (SIPG or membrane) neighbours outside the block in (cell, facet) order."""
    nblk = (nc_owned + B - 1) // B
    loc = np.zeros((nc_owned, 4), dtype=np.uint16)
    lists = [[] for _ in range(nblk)]
    for k in range(nc_owned):
        b = k // B
        for a in range(4):
            n = nbr_d[k, a]
            if kind_d[k, a] not in (oc.K_SIPG, oc.K_MEMBRANE) or n < 0:
                continue
            if n // B == b:
                loc[k, a] = n - b * B
            else:
                loc[k, a] = B + len(lists[b])
                lists[b].append(4 * n + nloc_d[k, a])
    return loc, lists


@pytest.mark.parametrize("which", ["2D_r0", "3D_4axon_r0", "emix"])
def test_device_connectivity_tables_bit_exact(hip_lib, which):
    mesh, sub, surf, mtags = _mesh(which)
    ctags, ftags = sub.array(), surf.array()
    exp = oc.derive_tables(mesh.cells, ctags, mesh.facets, ftags, mtags)
    dev = A.Device(mesh, ctags, ftags, mtags, 3)
    nc, nv = mesh.cells.shape
    meta = dev.debug_table(A.DT_META)
    assert meta[0] == nc and meta[1] == nc and meta[2] == mesh.num_facets() and meta[7] == mesh.gdim
    order, rank = dev.cell_order, dev.cell_rank                      # device -> caller, caller -> device
    assert np.array_equal(np.sort(order), np.arange(nc)) and np.array_equal(rank[order], np.arange(nc))

    # neighbours: device ids -> caller ids, rows -> caller rows
    nbr_d = dev.debug_table(A.DT_NBR).reshape(nc, nv).astype(np.int64)
    nbr_c = np.where(nbr_d >= 0, order[np.maximum(nbr_d, 0)], -1)
    assert np.array_equal(nbr_c, exp["nbr"][order])

    # flag bytes
    flag = dev.debug_table(A.DT_FLAG)
    fb = ((flag[:, None] >> (8 * np.arange(nv, dtype=np.uint32))[None, :]) & 0xFF).astype(np.int64)
    e = {k: v[order] for k, v in exp.items() if k != "mem"}
    assert np.array_equal((fb >> 2) & 3, e["kind"])
    assert np.array_equal(fb & 3, e["nloc"])
    assert np.array_equal((fb >> 4) & 1, e["plus"])
    assert not (fb >> 5).any()
    if nv == 3:
        assert not (flag >> 24).any()                                 # the unused fourth byte of a triangle

    # facet ids (caller numbering)
    assert np.array_equal(dev.debug_table(A.DT_CFACET).reshape(nc, nv), e["fid"])

    # membrane facets, in facet order
    mf = dev.debug_table(A.DT_MF).reshape(-1, 6).astype(np.int64)
    assert meta[3] == len(mf) == len(exp["mem"]) > 0
    em = np.array(exp["mem"], dtype=np.int64)
    assert np.array_equal(order[mf[:, 0]], em[:, 0]) and np.array_equal(order[mf[:, 1]], em[:, 1])
    assert np.array_equal(mf[:, 2:5], em[:, 2:5]) and (mf[:, 5] == 1).all()
    # plus side = lower subdomain tag (ECS-like) wherever the tags differ
    tp, tm = ctags[em[:, 0]].astype(np.int64), ctags[em[:, 1]].astype(np.int64)
    assert (tp <= tm).all()
    if which == "2D_r0":
        assert (tp == tm).any()               # too coarse for the ICS box: membrane-tagged facets between EQUAL-tag cells exercise the n('-') rule
    if which == "emix":
        assert set(np.unique(tm)) == {1, 2} and (tp == 0).all()      # glial and neuronal cells always face the ECS

    # cells: the caller's local vertex order (it carries the facet matching and the DoF numbering dof(c, a) = c * nd + a); only the
    # vertex STORAGE ids are relabelled
    cells_d = dev.debug_table(A.DT_CELLS).reshape(nc, nv)
    assert np.array_equal(cells_d, dev.vertex_rank[mesh.cells[order]])

    # halo-block tables of the 3D P1 apply
    src, loc = dev.debug_table(A.DT_HB_SRC), dev.debug_table(A.DT_HB_LOC)
    if nv == 4 and loc.size:
        hs, long0 = int(meta[4]), int(meta[5])
        eloc, lists = _expected_halo_tables(nbr_d, fb & 3, (fb >> 2) & 3, nc)
        nblk = (nc + 255) // 256
        assert long0 == next((b for b in range(nblk) if len(lists[b]) > 256), nblk)
        assert hs == (max(len(l) for l in lists[:long0]) + 7) // 8 * 8
        assert np.array_equal(loc.reshape(nc, 4), eloc)
        src = src.reshape(nblk, hs)
        for b in range(long0):
            L = lists[b]
            assert np.array_equal(src[b, :len(L)], np.array(L, dtype=np.int32)) and (src[b, len(L):] == -1).all()
    else:
        assert which == "2D_r0" and src.size == 0 and loc.size == 0
    dev.close()


def _expected_ring_u_tables(cells_d, nbr_d, nloc_d, kind_d, nc_owned, nblk_built, B=256, UH=320, UV=256):
    """Layout contract of KNP_DT_RU_* (include/knpemi_hip.h), restated for the first nblk_built blocks: per block the vertex list (own
    vertices of all its cells first, in (cell, local vertex) order of first appearance, then the apexes of the coupled neighbours in
    (cell, facet) order) and the list of coupled neighbours outside the block or not owned."""
    n = min(nblk_built * B, nc_owned)
    hb_src = np.full((nblk_built, UH), -1, dtype=np.int32)
    vb_src = np.zeros((nblk_built, UV), dtype=np.int32)
    hb_loc = np.zeros((n, 4), dtype=np.uint16)
    vloc = np.zeros((n, 8), dtype=np.uint8)
    coupled = np.zeros((n, 4), dtype=bool)
    nlist, nvert = [], []
    for b in range(nblk_built):
        pos, L = {}, []
        k0, k1 = b * B, min(nc_owned, (b + 1) * B)
        for k in range(k0, k1):
            for a in range(4):
                vloc[k, a] = pos.setdefault(int(cells_d[k, a]), len(pos))
        for k in range(k0, k1):
            for a in range(4):
                q = int(nbr_d[k, a])
                if kind_d[k, a] not in (oc.K_SIPG, oc.K_MEMBRANE) or q < 0:
                    continue
                coupled[k, a] = True
                j = int(nloc_d[k, a])
                vloc[k, 4 + a] = pos.setdefault(int(cells_d[q, j]), len(pos))
                if q // B == b and q < nc_owned:
                    hb_loc[k, a] = q - k0
                else:
                    hb_loc[k, a] = B + len(L)
                    L.append(4 * q + j)
        assert len(L) <= UH and len(pos) <= UV
        hb_src[b, :len(L)] = L
        vb_src[b, :len(pos)] = list(pos)
        nlist.append(len(L))
        nvert.append(len(pos))
    return hb_src, hb_loc, vb_src, vloc, coupled, np.array(nlist), np.array(nvert)


@pytest.mark.parametrize("which", ["emix", "C", "D1", "D6", "E_lists", "E_verts", "slab_of_12x4x4"])
def test_unstructured_ring_tables_bit_exact(hip_lib, monkeypatch, which):
    """The per-block tables of the unstructured ring-staged applies (csrc/apply_ring_u.hip: build_tables_u) entry for entry against
    the restated layout, their block counts against `block_stats` of tests/apply_split_cases.py -- which restates the builder from the
    MESH alone and is what the CPU test of the cases stands on -- and 2 / (h + h') against the oracle's cell diameters.  On the tissue
    mesh (every block fits) and on the cases with lists in the second DMA piece (C: 298 / 292 entries, LDS entries >= 512), a head that
    stops in front of an overflowing block (D1, D6), blocks exactly at and one past a limit (E_lists: 320 / 321 entries, E_verts:
    256 / 257 vertices) and an owned + ghost context whose ghosts fall into the id range of the last block (the `nbk < no` clause)."""
    import apply_split_cases as ac
    import knpemi_oracle as ko
    no = None
    if which == "emix":
        mesh, sub, surf, mtags = _mesh("emix")
        exp_meta = None
    elif which == "slab_of_12x4x4":
        lm, sub, surf = ac.partition_rank((12, 4, 4), "J", 0)[:3]
        mesh, mtags, no, exp_meta = lm.mesh, (1,), lm.nc_owned, None
    else:
        m, s, f = ac.base_mesh("J")
        mesh, sub, surf = ac.permuted_mesh(m, s, f, ac.case_order(which, m))
        mtags = (1,)
        monkeypatch.setenv("KNP_NO_REORDER", "1")
        exp_meta = ac.EXPECT[("J", which)][0]
    ctags, ftags = sub.array(), surf.array()
    dev = A.Device(mesh, ctags, ftags, mtags, 3, nc_owned=no)
    try:
        nc = mesh.num_cells()
        no = nc if no is None else no
        nblk = (no + 255) // 256
        order = dev.cell_order
        st = ac.block_stats(mesh, order, no, ftags, mtags)
        long0, hs = ac.expected_unstructured(st)
        assert exp_meta is None or (long0, hs) == exp_meta
        if which == "emix":
            assert long0 == nblk                                      # the tissue reconstruction in Morton order: every block fits
        if which == "slab_of_12x4x4":                                 # ghosts in the id range of the last block are staged through its list
            assert long0 == nblk == 3 and no == 576 < nc and st["lists_u"][2] > st["lists_s"][2]
        covered = min(long0 * 256, no)
        assert dev.n_geometry_classes == 0 and dev.apply_variant(0) == 10
        assert dev.debug_table(A.DT_RU_META).tolist() == [long0, hs, nblk, covered]
        nbr_d = dev.debug_table(A.DT_NBR).reshape(nc, 4).astype(np.int64)
        flag = dev.debug_table(A.DT_FLAG)
        fb = ((flag[:, None] >> (8 * np.arange(4, dtype=np.uint32))[None, :]) & 0xFF).astype(np.int64)
        cells_d = dev.debug_table(A.DT_CELLS).reshape(nc, 4)
        e_src, e_loc, e_vsrc, e_vloc, coupled, nlist, nvert = _expected_ring_u_tables(cells_d, nbr_d, fb & 3, (fb >> 2) & 3, no, long0)
        assert np.array_equal(nlist, st["lists_u"][:long0]) and np.array_equal(nvert, st["verts"][:long0])
        if long0 < nblk:
            assert st["lists_u"][long0] > 320 or st["verts"][long0] > 256
        src = dev.debug_table(A.DT_RU_HB_SRC).reshape(nblk, 320)
        loc = dev.debug_table(A.DT_RU_HB_LOC).reshape(no, 4)
        vsrc = dev.debug_table(A.DT_RU_VB_SRC).reshape(nblk, 256)
        vloc = dev.debug_table(A.DT_RU_VLOC).reshape(no, 8)
        hinv = dev.debug_table(A.DT_RU_HINV4).reshape(no, 4)
        assert np.array_equal(src[:long0], e_src) and np.array_equal(loc[:covered], e_loc)
        assert np.array_equal(vsrc[:long0], e_vsrc) and np.array_equal(vloc[:covered], e_vloc)
        if which == "C":
            assert sorted(np.nonzero(nlist > 256)[0].tolist()) == [5, 6] and (e_loc >= 512).any()
        if which == "E_verts":
            assert nvert[3] == 256 and (e_vloc[3 * 256:4 * 256] == 255).any()
        if which == "slab_of_12x4x4":                                 # a ghost behind an owned cell of the last block: a list entry, not an in-block one
            q = nbr_d[512:no]
            ghost = coupled[512:no] & (q >= no) & (q // 256 == 2)
            assert ghost.any() and (e_loc[512:no][ghost] >= 256).all()
        h = ko.Geometry(mesh).h[order]
        e_hinv = np.where(coupled, 2.0 / (h[:covered, None] + h[np.maximum(nbr_d[:covered], 0)]), 0.0)
        assert (np.abs(hinv[:covered] - e_hinv) <= 1e-15 * e_hinv).all()
    finally:
        dev.close()


def test_dof_layout_upload_download_bit_exact(hip_lib):
    """DoF layout: dof(c, a) = c * nd + a in the caller's numbering on both sides of the boundary, species-major
    for the KNP fields; the device's Morton order is invisible: what is uploaded comes back bit for bit, and a cell-indexed
    pattern lands on the cell it names (checked through the operator-free facet trace: plus / minus traces of a field whose
    value is the caller cell index return the indices of the oracle's plus / minus cells)."""
    mesh, sub, surf, mtags = _mesh("3D_4axon_r0")
    ctags, ftags = sub.array(), surf.array()
    exp = oc.derive_tables(mesh.cells, ctags, mesh.facets, ftags, mtags)
    dev = A.Device(mesh, ctags, ftags, mtags, 3)
    nc, nd = mesh.num_cells(), 4
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, nc, nd))
    dev.upload(A.F_C, x)
    assert np.array_equal(dev.download(A.F_C).reshape(2, nc, nd), x)
    ids = np.repeat(np.arange(nc, dtype=np.float64), nd)
    dev.upload(A.F_PHI, ids)
    em = np.array(exp["mem"], dtype=np.int64)
    for side, col in ((0, 0), (1, 1)):
        tr = dev.facet_trace(A.F_PHI, 0, side)
        got = tr[em[:, 4]]
        assert np.array_equal(np.rint(got), em[:, col].astype(np.float64)) and np.abs(got - np.rint(got)).max() < 1e-9
    dev.close()
