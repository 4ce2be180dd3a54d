"""Host side of the volume-field snapshots on the mesh (knpemidg/fieldmesh.py): the invariants of FieldMeshSpec on every case,
FieldMeshSpec.sample_host against an independent loop in extended precision (fieldmesh_cases.brute), every refusal, and the file
with its sidecar.  No device."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import fieldmesh_cases as FC
from knpemidg import fieldmesh as FM


def _id(v):
    return {True: "continuous", False: "dg"}.get(v, str(v)) if isinstance(v, bool) else str(v)


@pytest.mark.parametrize("name,p,sel,cont", FC.COMBOS, ids=_id)
def test_spec_invariants(name, p, sel, cont):
    mesh, sub, surf = FC.mesh_tuple(name)
    if FC.refused(name, sel, cont):
        with pytest.raises(ValueError, match="membrane facet .* separates two selected cells of tag 1"):
            FC.spec(name, p, sel, cont)
        return
    s = FC.spec(name, p, sel, cont)
    ct = np.asarray(sub.array()).astype(np.int64)
    cells = np.asarray(mesh.cells).astype(np.int64)
    d, nv = mesh.gdim, mesh.gdim + 1
    nd = nv if p == 1 else nv * (nv + 1) // 2
    want_cells = np.arange(len(cells)) if sel == "all" else np.nonzero(np.isin(ct, FC.ECS))[0]
    assert np.array_equal(s.cells, want_cells) and np.array_equal(s.tag, ct[want_cells]) and s.nd == nd and s.n_sel == len(want_cells)
    # every (selected cell, local dof) appears in exactly one list
    assert s.ptr[0] == 0 and s.ptr[-1] == len(s.cell) == len(s.dof) == s.n_sel * nd and (np.diff(s.ptr) >= 1).all()
    pair = s.cell * nd + s.dof
    assert len(np.unique(pair)) == len(pair) and np.array_equal(np.unique(s.cell), want_cells) and s.dof.min() == 0 and s.dof.max() == nd - 1
    node = np.repeat(np.arange(s.n_nodes), np.diff(s.ptr))
    # each list ascending by (cell, dof)
    inner = node[1:] == node[:-1]
    assert (np.diff(pair)[inner] > 0).all()
    # all entries of a list share the node's entity and tag, named here by vertex ids alone
    le = FM.local_edges(d)
    is_v = s.dof < nv
    assert np.array_equal(s.node_tag[node], ct[s.cell])
    assert np.array_equal(s.node_entity[node][is_v], cells[s.cell[is_v], s.dof[is_v]])
    if p == 2:
        ab = np.asarray(le)[s.dof[~is_v] - nv]
        ev = s.edge_vertices[s.node_entity[node][~is_v] - s.n_vertices]
        assert (s.node_entity[node][~is_v] >= s.n_vertices).all()
        assert np.array_equal(ev[:, 0], cells[s.cell[~is_v], ab[:, 0]]) and np.array_equal(ev[:, 1], cells[s.cell[~is_v], ab[:, 1]])
    # connectivity maps each cell's local dof to the node whose list contains it
    pos = np.searchsorted(want_cells, s.cell)
    assert s.connectivity.shape == (s.n_sel, nd) and np.array_equal(s.connectivity[pos, s.dof], node)
    # points: the vertex coordinates; edge nodes at the midpoint of the two vertex nodes the written order places them between
    assert s.points.shape == (s.n_nodes, 3) and (d == 3 or (s.points[:, 2] == 0.0).all())
    vnode = s.node_entity < s.n_vertices
    assert np.array_equal(s.points[vnode, :d], mesh.coords[s.node_entity[vnode]])
    xc = s.xdmf_connectivity()
    assert xc.shape == s.connectivity.shape and np.array_equal(xc[:, :nv], s.connectivity[:, :nv])
    if p == 2:
        assert np.array_equal(np.sort(xc[:, nv:], axis=1), np.sort(s.connectivity[:, nv:], axis=1))
        for j, (a, b) in enumerate(FC.VTK_EDGES[d]):
            assert np.array_equal(s.points[xc[:, nv + j]], 0.5 * (s.points[xc[:, a]] + s.points[xc[:, b]])), j
    else:
        assert xc is s.connectivity
    if cont:
        # one node per (entity, tag): the keys are distinct and are brute's; on a membrane vertex one node per adjacent tag
        keys = FC.node_keys(s)
        col = FC.brute(name, p, sel)[0]
        assert len(set(keys)) == len(keys) and set(keys) == set(col)
        if sel == "all":
            from knpemidg.recorder import membrane_facets
            mv = np.unique(mesh.facets[membrane_facets(mesh, np.asarray(surf.array()), FC.membrane_tags(name))])
            adjacent = {}
            for c in range(len(cells)):
                for v in cells[c]:
                    adjacent.setdefault(int(v), set()).add(int(ct[c]))
            per_vertex = np.bincount(s.node_entity[vnode], minlength=s.n_vertices)
            assert all(per_vertex[v] == len(adjacent[int(v)]) >= 2 for v in mv)
            assert all(per_vertex[v] == len(adjacent[v]) for v in adjacent)
    else:
        assert s.n_nodes == s.n_sel * nd and (np.diff(s.ptr) == 1).all()
        assert np.array_equal(s.connectivity.ravel(), np.arange(s.n_nodes))
    # with a cell_rank permutation: the same nodes and lists, matched by (entity, tag) resp. (cell, dof)
    r = FC.spec(name, p, sel, cont, ranked=True)
    assert r.n_nodes == s.n_nodes and np.array_equal(r.cells, s.cells)
    if cont:
        rk = {k: i for i, k in enumerate(FC.node_keys(r))}
        to_r = np.asarray([rk[k] for k in FC.node_keys(s)])
        assert not np.array_equal(to_r, np.arange(s.n_nodes))
    else:
        rpair = r.cell * nd + r.dof                        # lists of length one: entry i is node i
        by = np.argsort(rpair)
        to_r = by[np.searchsorted(rpair[by], pair)]
    assert np.array_equal(np.sort(to_r), np.arange(s.n_nodes))
    assert np.array_equal(r.node_entity[to_r], s.node_entity) and np.array_equal(r.node_tag[to_r], s.node_tag)
    assert np.array_equal(r.points[to_r], s.points) and np.array_equal(to_r[s.connectivity], r.connectivity)
    assert np.array_equal(np.diff(r.ptr)[to_r], np.diff(s.ptr))
    for i in (0, s.n_nodes // 2, s.n_nodes - 1):
        a, b = slice(s.ptr[i], s.ptr[i + 1]), slice(r.ptr[to_r[i]], r.ptr[to_r[i] + 1])
        assert np.array_equal(s.cell[a], r.cell[b]) and np.array_equal(s.dof[a], r.dof[b])
    # the ranked numbering follows the cell order: the first cell of the order holds the first nodes
    order = np.argsort(FC.stand_in_rank(len(cells)))
    first = int(order[np.isin(order, want_cells)][0])
    assert sorted(r.connectivity[np.searchsorted(want_cells, first)]) == list(range(nd))


@pytest.mark.parametrize("name,p,sel,cont", [c for c in FC.COMBOS if not FC.refused(c[0], c[2], c[3])], ids=_id)
def test_sample_host_against_the_independent_loop(name, p, sel, cont):
    """(The one combination without an output mesh is asserted to be refused in test_spec_invariants.)"""
    pb = FC.problem(name, p)
    s = FC.spec(name, p, sel, cont, ranked=True)
    fields = FC.fields_of(pb)
    got = s.sample_host(fields)
    assert list(got) == FC.field_names(pb) and all(v.shape == (s.n_nodes,) and v.dtype == np.float64 for v in got.values())
    if not cont:
        for q, u in fields.items():
            assert got[q].tobytes() == np.ascontiguousarray(u.reshape(len(u), -1)[s.cell, s.dof]).tobytes(), q      # bit for bit
        got32 = s.sample_host(fields, dtype=np.float32)
        assert all(got32[q].dtype == np.float32 and np.array_equal(got32[q], got[q].astype(np.float32)) for q in fields)
        return
    col, mean, scale, count = FC.brute(name, p, sel)
    at = np.asarray([col[k] for k in FC.node_keys(s)])
    assert np.array_equal(count[at], np.diff(s.ptr)) and count.max() > 1
    worst = 0.0
    for k, q in enumerate(FC.field_names(pb)):
        err = np.abs(got[q].astype(np.longdouble) - mean[k][at])
        bound = FC.BOUND * scale[k][at]
        assert (bound > 0).all()
        worst = max(worst, float((err / bound).max()))
    print("%s P%d %s: %d nodes, lists up to %d, largest error / bound %.3f" % (name, p, sel, s.n_nodes, count.max(), worst))
    assert worst < 1.0
    # discontinuous data: the mean differs from any single contribution on shared nodes
    shared = np.diff(s.ptr) > 1
    assert (got["phi"][shared] != fields["phi"].reshape(-1, s.nd)[s.cell[s.ptr[:-1]], s.dof[s.ptr[:-1]]][shared]).any()


def test_refusals_name_the_offender():
    ions = ["K", "Cl", "Na"]
    for bad, what in ((("phi", "c_Ca"), "c_Ca"), (("phi_M",), "'phi_M'"), (("phi", "c_K", "phi"), "'phi'.*twice"), ((), "no field"), ((3,), "3"),
                      (("K",), "'K'")):
        with pytest.raises(ValueError, match=what):
            FM.resolve_fields(bad, ions)
    assert FM.resolve_fields("phi", ions) == [(FM.FM_PHI, -1)]
    assert FM.resolve_fields(("c_Na", "phi", "c_K"), ions) == [(FM.FM_C, 2), (FM.FM_PHI, -1), (FM.FM_C, 0)]
    for kw, what in ((dict(tags=(7,)), "tag 7 is not a cell tag"), (dict(tags=(0, 0)), "tag 0 is listed twice"), (dict(tags=()), "no cell")):
        with pytest.raises(ValueError, match=what):
            FC.make_spec("3d", 1, **kw)
    with pytest.raises(ValueError, match="degree"):
        FC.make_spec("3d", 3)
    spec = lambda mtags, rank: FC.spec("3d", 1)
    for kw, what in ((dict(every=0), "every"), (dict(dtype=np.float16), "dtype"), (dict(dtype=np.int32), "dtype"), (dict(name=""), "name"),
                     (dict(name="a/b"), "name"), (dict(name="a" + os.sep + "b"), "name")):
        with pytest.raises(ValueError, match=what):
            FM.FieldSampler(spec, ["phi"], [(FM.FM_PHI, -1)], **kw)
    m = FM.FieldSampler(spec, ["phi"], [(FM.FM_PHI, -1)])
    assert m.dtype == np.float32 and m.every == 1 and m.name == "fields" and not m.attached


def test_a_same_tag_membrane_facet_is_refused():
    """The 3D mesh has none; retagging the ECS cell behind a membrane facet to the tag of the cell in front makes one.  On the 2D mesh
    every membrane facet is one already; retagging a cell there to a new tag takes the facets of that cell out, the others stay."""
    from knpemidg.recorder import membrane_facets
    mesh, sub, surf = FC.mesh_tuple("3d")
    ct = np.asarray(sub.array()).astype(np.int64)
    mf = membrane_facets(mesh, np.asarray(surf.array()), (1, 2))
    f = int(mf[40])
    a, b = (int(c) for c in mesh.facet_cells[f])
    assert ct[a] != ct[b]
    FC.make_spec("3d", 1)                                     # as it is: fine
    bad = ct.copy()
    bad[a] = bad[b] = max(ct[a], ct[b])
    with pytest.raises(ValueError, match=r"membrane facet \d+ separates two selected cells of tag %d" % max(ct[a], ct[b])):
        FC.make_spec("3d", 1, cell_tags=bad)
    assert FC.make_spec("3d", 1, cell_tags=bad, continuous=False).n_nodes == 4 * mesh.num_cells()       # the DG values need no mean
    assert FC.make_spec("3d", 1, cell_tags=bad, tags=(0,)).n_sel == (bad == 0).sum()                    # nor does a selection without them
    mesh2, sub2, surf2 = FC.mesh_tuple("2d")
    mf2 = membrane_facets(mesh2, np.asarray(surf2.array()), (1,))
    first = int(mf2[0])
    with pytest.raises(ValueError, match="membrane facet %d separates" % first):
        FC.make_spec("2d", 1)
    retagged = FC.one_cell_tags("2d", int(mesh2.facet_cells[first, 0]))
    with pytest.raises(ValueError, match=r"membrane facet (?!%d )\d+ separates" % first):
        FC.make_spec("2d", 1, cell_tags=retagged)
    assert FC.make_spec("2d", 1, cell_tags=retagged, tags=(7,)).n_sel == 1


@pytest.mark.parametrize("name,p,sel,dtype", [("2d", 1, "ecs", np.float32), ("2d", 2, "ecs", np.float64), ("3d", 1, "all", np.float32),
                                               ("3d", 2, "ecs", np.float64)], ids=_id)
def test_file_round_trip(tmp_path, name, p, sel, dtype):
    from knpemidg.h5lite import H5File
    s = FC.spec(name, p, sel, True, ranked=True)
    fields = ["phi", "c_K"]
    path = str(tmp_path / name / "fields.h5")
    f = FM.FieldMeshFile(path, s, fields, precision=np.dtype(dtype).itemsize)
    rng = np.random.default_rng(3)
    frames, times = [], [0.0, 2.5e-4, 5.0e-4]
    for k, t in enumerate(times):
        fr = {q: rng.uniform(-1, 1, s.n_nodes).astype(dtype) for q in fields}
        frames.append(fr)
        f.add(t, 2 * k, fr)
    assert not os.path.exists(path)                      # under its temporary name until close()
    assert f.close() == path and sorted(os.listdir(os.path.dirname(path))) == ["fields.h5", "fields.xdmf"]
    h = H5File(path)
    d, nd = s.dim, s.nd
    expect = {"mesh/points": ((s.n_nodes, 3), np.float64), "mesh/connectivity": ((s.n_sel, nd), np.int64), "mesh/cells": ((s.n_sel,), np.int64),
              "mesh/tag": ((s.n_sel,), np.int64), "mesh/node_entity": ((s.n_nodes,), np.int64), "mesh/node_tag": ((s.n_nodes,), np.int64),
              "t": ((3,), np.float64), "step": ((3,), np.int64)}
    for k in range(3):
        for q in fields:
            expect["%s/vector_%d" % (q, k)] = ((s.n_nodes,), np.dtype(dtype))
    assert sorted(h.datasets) == sorted(expect)
    for key, (shape, dt) in expect.items():
        a = h.read("/" + key)
        assert a.shape == shape and a.dtype == dt, key
    assert np.array_equal(h.read("/mesh/points"), s.points) and np.array_equal(h.read("/mesh/connectivity"), s.xdmf_connectivity())
    assert np.array_equal(h.read("/mesh/cells"), s.cells) and np.array_equal(h.read("/mesh/tag"), s.tag)
    assert np.array_equal(h.read("/mesh/node_entity"), s.node_entity) and np.array_equal(h.read("/mesh/node_tag"), s.node_tag)
    assert list(h.read("/t")) == times and list(h.read("/step")) == [0, 2, 4]
    for k in range(3):
        for q in fields:
            assert h.read("/%s/vector_%d" % (q, k)).tobytes() == frames[k][q].tobytes()
    # the sidecar
    root = ET.parse(os.path.splitext(path)[0] + ".xdmf").getroot()
    coll = root.find("Domain/Grid")
    assert coll.get("GridType") == "Collection" and coll.get("CollectionType") == "Temporal"
    grids = coll.findall("Grid")
    assert [float(g.find("Time").get("Value")) for g in grids] == times
    kinds = {(2, 1): "Triangle", (3, 1): "Tetrahedron", (2, 2): "Triangle_6", (3, 2): "Tetrahedron_10"}
    for k, g in enumerate(grids):
        topo, geo = g.find("Topology"), g.find("Geometry")
        assert topo.get("TopologyType") == kinds[(d, p)] and int(topo.get("NumberOfElements")) == s.n_sel and geo.get("GeometryType") == "XYZ"
        items = [(topo.find("DataItem"), "mesh/connectivity", "Int", 8), (geo.find("DataItem"), "mesh/points", "Float", 8)]
        attrs = g.findall("Attribute")
        assert [a.get("Name") for a in attrs] == ["tag"] + fields
        assert attrs[0].get("Center") == "Cell" and attrs[0].get("AttributeType") == "Scalar"
        items.append((attrs[0].find("DataItem"), "mesh/tag", "Int", 8))
        for a, q in zip(attrs[1:], fields):
            assert a.get("AttributeType") == "Scalar" and a.get("Center") == "Node"
            items.append((a.find("DataItem"), "%s/vector_%d" % (q, k), "Float", np.dtype(dtype).itemsize))
        for item, key, number, precision in items:
            fname, dset = item.text.strip().split(":/")
            assert fname == "fields.h5" and dset == key and dset in h.datasets
            assert item.get("Format") == "HDF" and item.get("NumberType") == number and int(item.get("Precision")) == precision
            a = h.read("/" + dset)
            assert tuple(int(x) for x in item.get("Dimensions").split()) == a.shape and a.dtype.itemsize == precision
            assert a.dtype.kind == ("i" if number == "Int" else "f")


def test_an_exception_before_close_leaves_no_file(tmp_path):
    s = FC.spec("2d", 1, "ecs", True)
    path = str(tmp_path / "fields.h5")

    def write():
        f = FM.FieldMeshFile(path, s, ["phi"], step_offset=4)
        f.add(0.0, 4, {"phi": np.zeros(s.n_nodes, dtype=np.float32)})
        f.add(1.0, 5, {"phi": np.zeros(s.n_nodes + 1, dtype=np.float32)})          # raises

    with pytest.raises(ValueError, match="one value per node"):
        write()
    assert not os.path.exists(path) and not os.path.exists(str(tmp_path / "fields.xdmf"))
    import gc
    gc.collect()
    assert os.listdir(str(tmp_path)) == []               # the temporary file went with the writer
    from knpemidg.h5lite import H5File
    f = FM.FieldMeshFile(path, s, ["phi"], step_offset=4)
    f.add(0.0, 4, {"phi": np.ones(s.n_nodes, dtype=np.float32)})
    f.close()
    assert list(H5File(path).read("/step_offset")) == [4] and list(H5File(path).read("/step")) == [4]
