"""Host side of the time-series recorder (knpemidg/recorder.py): point location and basis weights, the nodal weights of the
region integrals, facet selection and the errors of bad input.  No GPU needed."""
import itertools

import numpy as np
import pytest

from common import small_3d
from knpemidg.mesh import make_mesh_2D
from knpemidg import recorder as R
from quadrature import simplex_rule          # oracle/quadrature.py


def _meshes():
    return {"2d": make_mesh_2D(0), "3d": small_3d((7, 4, 4))}


MESHES = _meshes()


def _test_points(mesh, n=40, seed=0):
    """Random points inside the mesh, plus a vertex, a facet midpoint and a cell midpoint."""
    rng = np.random.default_rng(seed)
    lo, hi = mesh.coords.min(axis=0), mesh.coords.max(axis=0)
    pts = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(n, mesh.gdim))
    interior = mesh.interior_facets()
    extra = [mesh.coords[mesh.cells[5, 1]], mesh.facet_midpoints()[interior[3]], mesh.cell_midpoints()[7], mesh.coords[0], mesh.coords[-1]]
    return np.concatenate([pts, np.asarray(extra)])


def _brute_force(mesh, p, tol=1e-12):
    for c in range(mesh.num_cells()):
        X = mesh.coords[mesh.cells[c]]
        T = (X[1:] - X[0]).T
        lam = np.linalg.solve(T, p - X[0])
        lam = np.concatenate([[1.0 - lam.sum()], lam])
        if lam.min() >= -tol:
            return c, lam
    return None, None


def _nodes(mesh, cell, degree):
    X = mesh.coords[mesh.cells[cell]]
    if degree == 1:
        return X
    nv = len(X)
    return np.concatenate([X, [0.5 * (X[a] + X[b]) for a in range(nv) for b in range(a + 1, nv)]])


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_point_location_matches_brute_force(which):
    mesh = MESHES[which][0]
    pts = _test_points(mesh)
    cells, bary = R.locate_points(mesh, pts)
    for i, p in enumerate(pts):
        c, lam = _brute_force(mesh, p)
        assert c is not None
        assert cells[i] == c, "point %d: cell %d, brute force %d" % (i, cells[i], c)
        assert np.abs(bary[i] - lam).max() < 1e-12
        assert abs(bary[i].sum() - 1.0) < 1e-13


@pytest.mark.parametrize("which,degree", list(itertools.product(["2d", "3d"], [1, 2])))
def test_probe_weights_reproduce_polynomials(which, degree):
    """P1 weights reproduce a random affine function, P2 weights a random quadratic, exactly (1e-13 of the function's scale); both
    sum to 1."""
    mesh = MESHES[which][0]
    d = mesh.gdim
    pts = _test_points(mesh, seed=1)
    cells, bary = R.locate_points(mesh, pts)
    w = R.basis_weights(bary, degree)
    assert w.shape == (len(pts), d + 1 if degree == 1 else (d + 1) * (d + 2) // 2)
    assert np.abs(w.sum(axis=1) - 1.0).max() < 1e-13
    rng = np.random.default_rng(2)
    L = np.abs(mesh.coords).max(axis=0)                         # coordinates scaled to O(1) so that the coefficients are comparable
    a0, a1 = rng.uniform(-1, 1), rng.uniform(-1, 1, size=d)
    a2 = rng.uniform(-1, 1, size=(d, d)) if degree == 2 else np.zeros((d, d))

    def f(x):
        y = x / L
        return a0 + y @ a1 + np.einsum("...i,ij,...j->...", y, a2, y)
    scale = abs(a0) + np.abs(a1).sum() + np.abs(a2).sum()
    for i, p in enumerate(pts):
        u = f(_nodes(mesh, cells[i], degree))
        assert abs(w[i] @ u - f(p)) < 1e-13 * scale, (i, w[i] @ u, f(p))


def _lagrange_at(dim, degree, bary):
    """Nodal basis at barycentric points through a Vandermonde solve on the monomials of lambda_1 .. lambda_d (independent of the
    closed forms in recorder.basis_weights)."""
    nv = dim + 1
    nodes = [np.eye(nv)[a] for a in range(nv)]
    if degree == 2:
        nodes += [0.5 * (np.eye(nv)[a] + np.eye(nv)[b]) for a in range(nv) for b in range(a + 1, nv)]
    nodes = np.asarray(nodes)
    expo = [e for e in itertools.product(range(degree + 1), repeat=dim) if sum(e) <= degree]

    def mono(lam):
        return np.stack([np.prod(lam[:, 1:] ** np.asarray(e), axis=1) for e in expo], axis=1)
    V = mono(nodes)
    return mono(np.asarray(bary)) @ np.linalg.inv(V)


@pytest.mark.parametrize("dim,degree", list(itertools.product([2, 3], [1, 2])))
def test_region_nodal_weights_match_cell_quadrature(dim, degree):
    """vol * sum_a w_a u_a equals the oracle's cell quadrature of degree 2p applied to the nodal interpolant, for random nodal data."""
    w = R.nodal_integration_weights(dim, degree)
    nd = dim + 1 if degree == 1 else (dim + 1) * (dim + 2) // 2
    assert w.shape == (nd,) and abs(w.sum() - 1.0) < 1e-15
    bary, wq = simplex_rule(dim, 2 * degree)
    B = _lagrange_at(dim, degree, bary)                        # [nq, nd]
    rng = np.random.default_rng(3)
    mesh = MESHES["2d" if dim == 2 else "3d"][0]
    vol = R.cell_volumes(mesh)[:50]
    u = rng.uniform(-1, 1, size=(50, nd))
    got = vol * (u @ w)
    ref = vol * ((u @ B.T) @ wq)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    # the same through the volumes: they add up to the mesh's box
    ext = mesh.coords.max(axis=0) - mesh.coords.min(axis=0)
    assert abs(R.cell_volumes(mesh).sum() - np.prod(ext)) < 1e-12 * np.prod(ext)


def test_outside_point_raises():
    mesh, sub, surf = MESHES["3d"]
    hi = mesh.coords.max(axis=0)
    with pytest.raises(ValueError, match="point 1"):
        R.locate_points(mesh, [0.5 * hi, 1.5 * hi])
    with pytest.raises(ValueError, match="outside"):
        R.Recorder(mesh, sub.array(), surf.array(), 1, ["K", "Cl", "Na"], points=[-0.1 * hi], membrane_tags=[1])


def test_point_tags_pick_the_side_of_a_membrane():
    mesh, sub, surf = MESHES["3d"]
    mem = R.membrane_facets(mesh, surf.array(), [1])
    p = mesh.facet_midpoints()[mem[4]]
    tags = sub.array()
    for want in (0, 1):
        cells, bary = R.locate_points(mesh, [p], tags, [want])
        assert tags[cells[0]] == want and cells[0] in mesh.facet_cells[mem[4]]
    with pytest.raises(ValueError):
        R.locate_points(mesh, [p], tags, [7])


def test_box_selects_what_a_midpoint_loop_selects():
    mesh, sub, surf = MESHES["3d"]
    ft = surf.array()
    lo, hi = np.array([2.0e-6, 0.05e-6, 0.05e-6]), np.array([3.5e-6, 0.35e-6, 0.11e-6])
    want = []
    for f in range(mesh.num_facets()):
        x = mesh.coords[mesh.facets[f]].mean(axis=0)
        if ft[f] == 1 and mesh.facet_cells[f, 1] >= 0 and all(lo[k] <= x[k] <= hi[k] for k in range(3)):
            want.append(f)
    assert len(want) > 1
    rec = R.Recorder(mesh, sub.array(), ft, 1, ["K", "Cl", "Na"], membrane_sets=[(lo, hi), want[:1]], membrane_tags=[1])
    assert list(rec.set_facets[0]) == want
    assert list(rec.set_facets[1]) == want[:1]
    for w in rec.set_weights:
        assert abs(w.sum() - 1.0) < 1e-15 and (w > 0).all()
    assert rec.region_tags == [0, 1] and set(np.unique(rec.region)) == {0, 1}
    assert np.array_equal(rec.region == 1, sub.array() == 1)


def test_empty_or_foreign_membrane_set_raises():
    mesh, sub, surf = MESHES["3d"]
    far = (np.array([100.0, 100.0, 100.0]), np.array([101.0, 101.0, 101.0]))
    with pytest.raises(ValueError, match="empty"):
        R.Recorder(mesh, sub.array(), surf.array(), 1, ["K", "Cl", "Na"], membrane_sets=[far], membrane_tags=[1])
    with pytest.raises(ValueError, match="empty"):
        R.Recorder(mesh, sub.array(), surf.array(), 1, ["K", "Cl", "Na"], membrane_sets=[np.zeros(0, dtype=np.int64)], membrane_tags=[1])
    not_mem = int(np.nonzero(surf.array() == 0)[0][0])
    with pytest.raises(ValueError, match="not a membrane facet"):
        R.Recorder(mesh, sub.array(), surf.array(), 1, ["K", "Cl", "Na"], membrane_sets=[[not_mem]], membrane_tags=[1])


def test_recorder_module_does_not_reach_for_the_oracle():
    import os
    src = open(os.path.join(os.path.dirname(R.__file__), "recorder.py")).read()
    assert "knpemi_oracle" not in src and "oracle" + "/" not in src


def test_save_writes_the_named_series(tmp_path):
    """Recorder.save / h5lite round trip on rows put there by hand (the device fills them in a real run)."""
    from knpemidg.h5lite import H5File
    mesh, sub, surf = MESHES["2d"]
    mem = R.membrane_facets(mesh, surf.array(), [1])
    mid = mesh.cell_midpoints()
    rec = R.Recorder(mesh, sub.array(), surf.array(), 2, ["K", "Cl", "Na"], points=[mid[3], mid[100]], membrane_sets=[mem[:4]],
                     membrane_tags=[1])
    n_ch = 2 * 4 + 7 + 2 * 4
    rec.n_channels = n_ch
    rows = np.arange(5 * n_ch, dtype=np.float64).reshape(5, n_ch)
    rec._rows, rec._t = [rows[:3], rows[3:]], [np.arange(3.0), np.arange(3.0, 5.0)]
    assert np.array_equal(rec.t, np.arange(5.0)) and np.array_equal(rec.rows, rows)
    assert np.array_equal(rec.points["phi"], rows[:, [0, 4]]) and np.array_equal(rec.points["Na"], rows[:, [3, 7]])
    assert np.array_equal(rec.membrane["I_ch_Na"][:, 0], rows[:, 8 + 6])
    assert np.array_equal(rec.regions["phi_mean"], rows[:, [15 + 3, 15 + 7]])
    h = H5File(rec.save(str(tmp_path / "ts.h5")))
    assert np.array_equal(h.read("timeseries/t"), np.arange(5.0))
    assert np.array_equal(h.read("timeseries/points/K"), rec.points["K"])
    assert np.array_equal(h.read("timeseries/membrane/phi_M"), rec.membrane["phi_M"])
    assert np.array_equal(h.read("timeseries/regions/Cl"), rec.regions["Cl"])
    assert np.array_equal(h.read("probes/coordinates"), np.asarray([mid[3], mid[100]]))
    assert np.array_equal(h.read("membrane_sets/set_0/facets"), mem[:4]) and list(h.read("regions/tags")) == [0, 1]
