"""Host side of the voxel-grid sampler (knpemidg/grid.py): the vectorised locate against recorder.locate_points, the host sample
against basis_weights(barycentric) @ u, the frame file read back with h5lite and its XDMF sidecar parsed with xml.etree, and what
is refused.  No GPU."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import grid_cases as G
from knpemidg import recorder as R
from knpemidg.grid import GridFile, GridSpec, resolve_fields
from knpemidg.h5lite import H5File

CASES = [("2d", "generic"), ("2d", "exact"), ("3d", "generic"), ("3d", "exact"), ("emix", "generic")]


@pytest.mark.parametrize("name,kind", CASES)
def test_host_locate_gives_the_owners_of_locate_points(name, kind):
    """Every point with an owner goes through ONE locate_points call (it must not raise, and must name the same cells and the same
    barycentric coordinates to rounding).  A point without one must make locate_points raise, in a call of its own: every such
    point in 2D, every 5th in 3D (locate_points rebuilds the bounding boxes of all cells on every call, 2 ms at 15 k cells).  ALL
    points are then checked against the brute-force candidates, which restate locate_points' rule with its own arithmetic."""
    mesh = G.mesh_tuple(name)[0]
    s = G.spec(name, kind)
    owner, bary, cells, lam = G.located(name, kind)
    pts = s.points()
    found = owner >= 0
    if kind == "generic":
        assert found.sum() == G.SHAPES[name][1] and s.npts == int(np.prod(G.SHAPES[name][0]))
    else:
        assert found.all()
    assert np.array_equal(cells, owner[found])
    assert np.abs(lam - bary[found]).max() < 1e-9
    assert (bary[~found] == 0.0).all()
    outside = np.nonzero(~found)[0]
    for i in outside[::1 if mesh.gdim == 2 else 5]:
        with pytest.raises(ValueError, match="outside the mesh"):
            R.locate_points(mesh, pts[i][None])
    pi, ci, cl = G.candidates(name, kind)
    assert np.array_equal(owner, G.owners_from_candidates(s.npts, pi, ci, cl))
    if kind == "exact":
        several = np.bincount(pi[cl.min(axis=1) >= -1e-12], minlength=s.npts) > 1
        assert several.sum() == G.SHAPES[name][3]


@pytest.mark.parametrize("name,kind,p", [("2d", "generic", 1), ("2d", "exact", 2), ("3d", "generic", 2), ("emix", "generic", 1)])
def test_host_sample_is_basis_weights_times_nodal_values(name, kind, p):
    mesh = G.mesh_tuple(name)[0]
    s = G.spec(name, kind)
    owner, bary, cells, lam = G.located(name, kind)
    nd = R.basis_weights(np.zeros((1, mesh.gdim + 1)), p).shape[1]
    u = np.random.default_rng(5).uniform(-1, 1, size=(mesh.num_cells(), nd))
    got = s.sample(u, p, owner, bary)
    found = owner >= 0
    assert np.isnan(got[~found]).all() and np.isfinite(got[found]).all()
    pts = s.points()
    want = np.einsum("ia,ia->i", R.basis_weights(lam, p), u[cells])
    bound = G.value_bound(mesh, pts, owner, u)[found]
    ratio = np.abs(got[found] - want) / bound
    print("%s %s P%d: largest error / bound %.2e" % (name, kind, p, ratio.max()))
    assert ratio.max() < 1.0


def test_tags_restrict_the_candidates_and_a_slice_is_a_plane_of_its_volume():
    mesh, sub, _ = G.mesh_tuple("3d")
    tags = np.asarray(sub.array())
    lo, hi = G.exact_bounds(mesh)
    # 33 x 9 x 9 is the coarsest of these grids with points ON the membrane (32 of them; 17 x 9 x 9 has none)
    vol = GridSpec(3, lo, hi, (33, 9, 9))
    ics = GridSpec(3, lo, hi, (33, 9, 9), tags=(1,))
    ecs = GridSpec(3, lo, hi, (33, 9, 9), tags=(0,))
    o_all, _ = vol.locate(mesh)
    o_ics, _ = ics.locate(mesh, tags)
    o_ecs, _ = ecs.locate(mesh, tags)
    found = o_ics >= 0
    assert found.any() and not found.all() and (tags[o_ics[found]] == 1).all()
    pts = vol.points()
    want = R.locate_points(mesh, pts[found], tags, np.ones(found.sum(), dtype=np.int64))[0]
    assert np.array_equal(o_ics[found], want)
    # points on the membrane have a cell on both sides; without the filter the lower index wins, which is extracellular for some
    on_membrane = found & (o_ecs >= 0)
    assert on_membrane.sum() == 32 and (np.minimum(o_ics, o_ecs)[on_membrane] == o_all[on_membrane]).all()
    assert (o_all[on_membrane] != o_ics[on_membrane]).sum() == 16
    assert ((o_ics >= 0) | (o_ecs >= 0)).all()
    with pytest.raises(ValueError, match="cell tags"):
        ics.locate(mesh)
    vol = GridSpec(3, lo, hi, (17, 9, 9))
    o_all, _ = vol.locate(mesh)
    k = 4
    z = lo[2] + k * vol.h[2]
    plane = GridSpec(3, (lo[0], lo[1], z), (hi[0], hi[1], z), (17, 9, 1))
    o_pl, b_pl = plane.locate(mesh)
    assert plane.array_shape == (1, 9, 17)
    assert np.array_equal(o_pl.reshape(9, 17), o_all.reshape(9, 9, 17)[k])
    assert np.array_equal(b_pl, vol.bary.reshape(9, 9, 17, 4)[k].reshape(-1, 4))


@pytest.mark.parametrize("name,dtype", [("2d", np.float64), ("3d", np.float32)])
def test_frame_file_round_trip_and_sidecar(tmp_path, name, dtype):
    mesh, sub, _ = G.mesh_tuple(name)
    s = G.spec(name, "generic")
    owner, _ = s.locate(mesh)
    tag = np.where(owner >= 0, np.asarray(sub.array()).astype(np.int64)[np.maximum(owner, 0)], -1)
    rng = np.random.default_rng(3)
    fields = ["phi", "K"]
    path = str(tmp_path / "out" / "grid.h5")
    gf = GridFile(path, s, fields, owner, tag, step_offset=0)
    assert not os.path.exists(path)                       # written under a temporary name until close()
    frames = []
    for n in range(3):
        fr = {f: s.sample(rng.uniform(-1, 1, size=(mesh.num_cells(), mesh.gdim + 1)), 1).astype(dtype).reshape(s.array_shape) for f in fields}
        gf.add(0.5 * n, 5 * n, fr)
        frames.append(fr)
    assert gf.close() == path
    assert sorted(os.listdir(tmp_path / "out")) == ["grid.h5", "grid.xdmf"]
    h = H5File(path)
    assert np.array_equal(h.read("/grid/lo"), s.lo) and np.array_equal(h.read("/grid/hi"), s.hi)
    assert np.array_equal(h.read("/grid/shape"), s.shape) and np.array_equal(h.read("/grid/spacing"), s.h)
    assert np.array_equal(h.read("/grid/cell"), owner.reshape(s.array_shape))
    assert np.array_equal(h.read("/grid/tag"), tag.reshape(s.array_shape))
    assert list(h.read("/t")) == [0.0, 0.5, 1.0] and list(h.read("/step")) == [0, 5, 10]
    for n, fr in enumerate(frames):
        for f in fields:
            a = h.read("/%s/vector_%d" % (f, n))
            assert a.dtype == np.dtype(dtype) and a.shape == s.array_shape
            assert np.array_equal(a, fr[f], equal_nan=True)
    root = ET.parse(str(tmp_path / "out" / "grid.xdmf")).getroot()
    coll = root.find("Domain/Grid")
    assert coll.get("GridType") == "Collection" and coll.get("CollectionType") == "Temporal"
    grids = coll.findall("Grid")
    assert [float(g.find("Time").get("Value")) for g in grids] == [0.0, 0.5, 1.0]
    dims = " ".join(str(n) for n in s.array_shape)
    seen = 0
    for g in grids:
        topo = g.find("Topology")
        assert topo.get("TopologyType") == ("3DCoRectMesh" if s.dim == 3 else "2DCoRectMesh") and topo.get("Dimensions") == dims
        geo = g.find("Geometry")
        assert geo.get("GeometryType") == ("ORIGIN_DXDYDZ" if s.dim == 3 else "ORIGIN_DXDY")
        origin, spacing = [np.array(x.text.split(), dtype=np.float64) for x in geo.findall("DataItem")]
        assert np.array_equal(origin, s.lo[::-1]) and np.array_equal(spacing, s.h[::-1])        # z-y-x order
        for item in g.iter("DataItem"):
            if item.get("Format") != "HDF":
                continue
            fname, dset = item.text.strip().split(":")
            assert fname == "grid.h5"
            a = H5File(str(tmp_path / "out" / fname)).read(dset)
            assert " ".join(str(n) for n in a.shape) == item.get("Dimensions") == dims
            assert int(item.get("Precision")) == a.dtype.itemsize
            seen += 1
    assert seen == 3 * len(fields)


def test_a_resumed_part_carries_its_step_offset(tmp_path):
    mesh = G.mesh_tuple("2d")[0]
    s = G.spec("2d", "generic")
    owner, _ = s.locate(mesh)
    gf = GridFile(str(tmp_path / "grid_from4.h5"), s, ["phi"], owner, owner, step_offset=4)
    gf.add(0.4, 4, {"phi": np.zeros(s.array_shape)})
    gf.close()
    h = H5File(str(tmp_path / "grid_from4.h5"))
    assert list(h.read("/step_offset")) == [4] and list(h.read("/step")) == [4]
    assert os.path.exists(tmp_path / "grid_from4.xdmf")


def test_refusals():
    ok = dict(lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), shape=(4, 4, 4))
    GridSpec(3, **ok)
    for change in (dict(shape=(4, 4)), dict(shape=(4, 0, 4)), dict(shape=(4, 4, -1)), dict(shape=(2048, 2048, 512)), dict(shape=(4, 4.5, 4)),
                   dict(lo=(0.0, np.nan, 0.0)), dict(hi=(1.0, 1.0, np.inf)), dict(hi=(1.0, 0.0, 1.0)), dict(lo=(0.0, 0.0))):
        with pytest.raises(ValueError):
            GridSpec(3, **dict(ok, **change))
    GridSpec(3, (0.0, 0.0, 0.5), (1.0, 1.0, 0.5), (4, 4, 1))       # a slice: one point along z, hi == lo there
    with pytest.raises(ValueError):
        GridSpec(3, tol=-1.0, **ok)
    with pytest.raises(ValueError):
        GridSpec(3, tags=tuple(range(9)), **ok)
    ions = ["K", "Cl", "Na"]
    assert resolve_fields(("phi", "Na", "K"), ions) == [0, 3, 1] and resolve_fields("Cl", ions) == [2]
    for bad in (("phi", "Ca"), ("c",), (), ("K", "K")):
        with pytest.raises(ValueError):
            resolve_fields(bad, ions)
