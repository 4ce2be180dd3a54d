"""Host side of the membrane-surface snapshots (knpemidg/surface.py): SurfaceSpec.sample_host against an independent brute-force
statement (surface_cases.brute_trace), the geometry of the surface mesh, the file and its sidecar, and every refusal.  No device.
(pcws_constant_project has no host-side definition -- it runs knp_facet_trace -- so that comparison is in tests/test_gpu_surface.py.)"""
import os
import xml.etree.ElementTree as ET
from types import SimpleNamespace

import numpy as np
import pytest

import surface_cases as SC
from knpemidg import recorder as R
from knpemidg import surface as SF


@pytest.mark.parametrize("name,p", SC.CASES)
def test_sample_host_against_the_brute_force_statement(name, p):
    """Every plane of every field name; traces within 8 eps sum |w_a u_a| of the quadrature statement, facet planes the exact values
    of the facet arrays, I_ch_total the sum in ion order."""
    mesh, sub, surf = SC.mesh_tuple(name)
    pb = SC.problem(name, p)
    s = SC.spec(name, p)
    assert s.n == len(pb.mem) and np.array_equal(s.facets, np.sort(pb.mem))
    names = SC.all_fields(pb)
    ids = SF.resolve_fields(names, SC.ion_names(pb))
    phi_M, E, I = SC.facet_arrays(pb)
    nodal = SC.nodal_fields(pb)
    got = s.sample_host(list(zip(names, ids)), phi_M=phi_M, E=E, I_ch=I, phi=nodal[0], conc=nodal[1:])
    assert list(got) == names
    assert got["phi_M"].tobytes() == phi_M[s.facets].tobytes()
    total = I[0][s.facets].copy()
    for k, ion in enumerate(SC.ion_names(pb)):
        assert got["E_" + ion].tobytes() == E[k][s.facets].tobytes()
        assert got["I_ch_" + ion].tobytes() == I[k][s.facets].tobytes()
        if k:
            total = total + I[k][s.facets]
    assert got["I_ch_total"].tobytes() == total.tobytes()
    worst = 0.0
    traced = [("phi", nodal[0])] + [("c_" + ion, nodal[1 + k]) for k, ion in enumerate(SC.ion_names(pb))]
    for base, u in traced:
        sides = []
        for side, suffix in ((0, "_e"), (1, "_i")):
            want, scale = SC.brute_trace(mesh, sub.array(), s.facets, u, p, side)
            mean, my_scale = s.trace(u, side)
            assert np.array_equal(mean, got[base + suffix])
            assert np.allclose(my_scale, scale, rtol=1e-12, atol=0.0)
            ratio = np.abs(mean - want) / (SC.BOUND * scale)
            worst = max(worst, float(ratio.max()))
            sides.append(mean)
        assert not np.array_equal(sides[0], sides[1])           # discontinuous data: the two sides differ
    print("%s P%d: %d facets, largest error / bound %.3f" % (name, p, s.n, worst))
    assert worst < 1.0


def test_trace_weights_are_the_exact_facet_means():
    """The compile-time weights against the quadrature of the nodal basis: P1 and P2, 2D and 3D, every local facet."""
    from knpemidg.quadrature import simplex_rule
    for d in (2, 3):
        for p in (1, 2):
            w = SF.trace_weights(d, p)
            pts, wq = simplex_rule(d - 1, 2)
            for l in range(d + 1):
                lam = np.zeros((len(wq), d + 1))
                lam[:, [a for a in range(d + 1) if a != l]] = pts
                want = (wq[:, None] * R.basis_weights(lam, p)).sum(axis=0)
                assert np.abs(w[l] - want).max() < 1e-15, (d, p, l)
                assert abs(w[l].sum() - 1.0) < 1e-15


@pytest.mark.parametrize("name", ["2d", "3d", "emix"])
def test_geometry_of_the_surface_mesh(name):
    mesh, sub, surf = SC.mesh_tuple(name)
    s = SC.spec(name, 1)
    d = mesh.gdim
    # compaction: a bijection onto the used vertices
    used = np.unique(mesh.facets[s.facets])
    assert np.array_equal(s.vertices, used) and len(s.points) == len(used)
    assert np.array_equal(np.unique(s.connectivity), np.arange(len(used)))
    assert s.connectivity.shape == (s.n, d) and s.points.shape[1] == 3
    assert np.array_equal(s.points[:, :d], mesh.coords[used]) and (d == 3 or (s.points[:, 2] == 0.0).all())
    # the same vertex set per facet as the mesh's facet table
    assert np.array_equal(np.sort(s.vertices[s.connectivity], axis=1), np.sort(mesh.facets[s.facets], axis=1))
    # the normal points from the _i cell to the _e cell
    centre = mesh.coords[mesh.cells[s.cells]].mean(axis=2)
    out = centre[:, 0] - centre[:, 1]
    assert (np.einsum("nd,nd->n", s.normals()[:, :d], out) > 0.0).all()
    # sides: _e is the lower cell tag, the two cells are the facet's
    ct = np.asarray(sub.array()).astype(np.int64)
    assert (ct[s.cells[:, 0]] <= ct[s.cells[:, 1]]).all()
    rows = np.arange(s.n)
    assert np.array_equal(s.cells[:, 0], mesh.facet_cells[s.facets][rows, SC.e_side(mesh, ct, s.facets)])
    assert np.array_equal(np.sort(s.cells, axis=1), np.sort(mesh.facet_cells[s.facets], axis=1))
    assert np.array_equal(s.area, R.facet_areas(mesh, s.facets))
    assert np.array_equal(s.tags, np.asarray(surf.array())[s.facets]) and (np.diff(s.facets) > 0).all()


def test_selections():
    mesh, sub, surf = SC.mesh_tuple("3d")
    ft = np.asarray(surf.array())
    allmf = R.membrane_facets(mesh, ft, (1, 2))
    s2 = SC.spec("3d", 1, (2,))
    assert np.array_equal(s2.facets, allmf[ft[allmf] == 2]) and 0 < s2.n < len(allmf)
    one = SF.SurfaceSpec(mesh, surf, sub, (1, 2), facets=[int(allmf[17])])
    assert one.n == 1 and one.facets[0] == allmf[17]
    rest = SF.SurfaceSpec(mesh, surf, sub, (1, 2), facets=list(allmf[1:][::-1]))          # given descending: kept ascending
    assert np.array_equal(rest.facets, allmf[1:])


def test_file_round_trip(tmp_path):
    from knpemidg.h5lite import H5File
    for name, dtype in (("3d", np.float64), ("2d", np.float32)):
        s = SC.spec(name, 1)
        planes = ["phi_M", "c_K_e", "n"]
        path = str(tmp_path / name / "membrane.h5")
        f = SF.SurfaceFile(path, s, planes, precision=np.dtype(dtype).itemsize)
        rng = np.random.default_rng(3)
        frames, times = [], [0.0, 2.5e-4, 5.0e-4]
        for k, t in enumerate(times):
            fr = {q: rng.uniform(-1, 1, s.n).astype(dtype) for q in planes}
            fr["n"][::3] = np.nan
            frames.append(fr)
            f.add(t, 2 * k, fr)
        assert not os.path.exists(path)                      # under its temporary name until close()
        assert f.close() == path and sorted(os.listdir(os.path.dirname(path))) == ["membrane.h5", "membrane.xdmf"]
        h = H5File(path)
        d = s.dim
        expect = {"surface/points": ((len(s.points), 3), np.float64), "surface/connectivity": ((s.n, d), np.int64),
                  "surface/facet": ((s.n,), np.int64), "surface/tag": ((s.n,), np.int64), "surface/cells": ((s.n, 2), np.int64),
                  "surface/area": ((s.n,), np.float64), "t": ((3,), np.float64), "step": ((3,), np.int64)}
        for k in range(3):
            for q in planes:
                expect["%s/vector_%d" % (q, k)] = ((s.n,), np.dtype(dtype))
        assert sorted(h.datasets) == sorted(expect)
        for key, (shape, dt) in expect.items():
            a = h.read("/" + key)
            assert a.shape == shape and a.dtype == dt, key
        assert np.array_equal(h.read("/surface/points"), s.points) and np.array_equal(h.read("/surface/connectivity"), s.connectivity)
        assert np.array_equal(h.read("/surface/facet"), s.facets) and np.array_equal(h.read("/surface/cells"), s.cells)
        assert np.array_equal(h.read("/surface/area"), s.area) and np.array_equal(h.read("/surface/tag"), s.tags)
        assert list(h.read("/t")) == times and list(h.read("/step")) == [0, 2, 4]
        for k in range(3):
            for q in planes:
                assert h.read("/%s/vector_%d" % (q, k)).tobytes() == frames[k][q].tobytes()
        # the sidecar
        root = ET.parse(os.path.splitext(path)[0] + ".xdmf").getroot()
        coll = root.find("Domain/Grid")
        assert coll.get("GridType") == "Collection" and coll.get("CollectionType") == "Temporal"
        grids = coll.findall("Grid")
        assert [float(g.find("Time").get("Value")) for g in grids] == times
        for k, g in enumerate(grids):
            topo, geo = g.find("Topology"), g.find("Geometry")
            if d == 3:
                assert topo.get("TopologyType") == "Triangle"
            else:
                assert topo.get("TopologyType") == "Polyline" and topo.get("NodesPerElement") == "2"
            assert int(topo.get("NumberOfElements")) == s.n and geo.get("GeometryType") == "XYZ"
            items = [(topo.find("DataItem"), "surface/connectivity"), (geo.find("DataItem"), "surface/points")]
            attrs = g.findall("Attribute")
            assert [a.get("Name") for a in attrs] == planes
            for a, q in zip(attrs, planes):
                assert a.get("AttributeType") == "Scalar" and a.get("Center") == "Cell"
                assert a.find("DataItem").get("Precision") == str(np.dtype(dtype).itemsize)
                items.append((a.find("DataItem"), "%s/vector_%d" % (q, k)))
            for item, key in items:
                fname, dset = item.text.strip().split(":/")
                assert fname == "membrane.h5" and dset == key and dset in h.datasets
                assert tuple(int(x) for x in item.get("Dimensions").split()) == h.read("/" + dset).shape


def _model(facets, ode, handle):
    return SimpleNamespace(facets=np.asarray(facets), ode=ode, handle=handle)


def test_state_tables():
    from knpemidg.models import mm_hh, mm_leak
    mesh, sub, surf = SC.mesh_tuple("3d")
    ft = np.asarray(surf.array())
    s = SC.spec("3d", 1)
    f1, f2 = R.membrane_facets(mesh, ft, (1,)), R.membrane_facets(mesh, ft, (2,))
    models = [_model(f1, mm_hh, 0), _model(f2, mm_leak, 1)]
    handle, row, col = s.state_tables(models, ["n", "V"])
    on1 = np.isin(s.facets, f1)
    assert (handle[0][on1] == 0).all() and (handle[0][~on1] == -1).all()           # mm_leak has no n
    assert (handle[1][on1] == 0).all() and (handle[1][~on1] == 1).all()
    assert np.array_equal(f1[row[0][on1]], s.facets[on1]) and np.array_equal(f2[row[1][~on1]], s.facets[~on1])
    assert (col[0][on1] == mm_hh.state_indices("n")).all() and (col[1][~on1] == mm_leak.state_indices("V")).all()
    tables = {0: np.random.default_rng(0).uniform(size=(len(f1), 4)), 1: np.random.default_rng(1).uniform(size=(len(f2), 1))}
    got = s.sample_host([], states=[("n", handle[0], row[0], col[0])], state_tables=tables)["n"]
    assert np.array_equal(np.isnan(got), ~on1)
    assert np.array_equal(got[on1], tables[0][:, mm_hh.state_indices("n")][np.searchsorted(f1, s.facets[on1])])
    with pytest.raises(ValueError, match="'q'"):
        s.state_tables(models, ["n", "q"])
    with pytest.raises(ValueError, match="'n'"):
        SC.spec("3d", 1, (2,)).state_tables(models, ["n"])                         # no selected facet has it


def test_refusals_name_the_offender():
    mesh, sub, surf = SC.mesh_tuple("3d")
    ft = np.asarray(surf.array())
    ions = ["Na", "K", "Cl"]
    for bad, what in ((("phi_M", "E_Ca"), "E_Ca"), (("phi",), "'phi'"), (("phi_M", "c_K_e", "phi_M"), "'phi_M'.*twice"), ((), "no field"),
                      ((3,), "3")):
        with pytest.raises(ValueError, match=what):
            ids = SF.resolve_fields(bad, ions)
            SF.check_names(bad, ())
    with pytest.raises(ValueError, match="'total'"):
        SF.resolve_fields(("phi_M",), ["Na", "total"])
    assert SF.resolve_fields("I_ch_total", ions) == [(SF.SF_I_CH_TOTAL, -1)]
    assert SF.resolve_fields(("c_Cl_i", "phi_e", "E_Na"), ions) == [(SF.SF_TRACE_I, 2), (SF.SF_TRACE_E, -1), (SF.SF_E, 0)]
    with pytest.raises(ValueError, match="'n'.*twice"):
        SF.check_names(["phi_M"], ["n", "n"])
    with pytest.raises(ValueError, match="name of a field"):
        SF.check_names(["phi_M"], ["phi_M"])
    assert SF.check_names([], ["n"]) == ["n"]
    allmf = R.membrane_facets(mesh, ft, (1, 2))
    interior = np.nonzero((mesh.facet_cells[:, 1] >= 0) & (ft == 0))[0]
    exterior = np.nonzero(mesh.facet_cells[:, 1] < 0)[0]
    mk = lambda **kw: SF.SurfaceSpec(mesh, surf, sub, (1, 2), **kw)
    for kw, what in ((dict(facets=[int(allmf[0]), int(interior[0])]), "facet %d is not a membrane" % interior[0]),
                     (dict(facets=[int(exterior[0])]), "facet %d is not a membrane" % exterior[0]),
                     (dict(facets=[-1]), "facet -1"), (dict(facets=[mesh.num_facets()]), "facet %d" % mesh.num_facets()),
                     (dict(facets=[int(allmf[3]), int(allmf[3])]), "facet %d is listed twice" % allmf[3]),
                     (dict(facets=[]), "no facet"), (dict(facets=[1.5]), "whole"), (dict(tags=(7,)), "tag 7"),
                     (dict(tags=(1, 1)), "tag 1 is listed twice"), (dict(tags=()), "no facet"),
                     (dict(tags=(1,), facets=[int(allmf[0])]), "mutually exclusive")):
        with pytest.raises(ValueError, match=what):
            mk(**kw)
    assert SF.SurfaceSpec(mesh, surf, sub, (1,), tags=None).n == (ft[allmf] == 1).sum()        # tag 2 is no membrane here
    with pytest.raises(ValueError, match="tag 2 is not a membrane tag"):
        SF.SurfaceSpec(mesh, surf, sub, (1,), tags=(2,))
    spec = lambda mt: mk()
    for kw, what in ((dict(every=0), "every"), (dict(dtype=np.float16), "dtype"), (dict(name=""), "name"), (dict(name="a/b"), "name")):
        with pytest.raises(ValueError, match=what):
            SF.MembraneSampler(spec, ["phi_M"], [(SF.SF_PHI_M, -1)], **kw)
