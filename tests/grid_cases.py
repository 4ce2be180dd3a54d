"""Meshes, grids and host references shared by tests/test_grid_host.py and tests/test_gpu_grid.py.

`candidates` is an independent brute-force statement of recorder.locate_points' rule: for every grid point the cells whose padded
bounding box contains it and the barycentric coordinates there, solved as recorder.barycentric solves them (np.linalg.solve on the
edge matrix).  Everything here is computed once per mesh and grid (lru_cache) and never changed."""
import functools

import numpy as np

LO_FRAC = np.array([0.0371, 0.0419, 0.0287])
HI_FRAC = np.array([0.0533, 0.0611, 0.0477])

# mesh name -> (generic-position shape, points inside, exact-grid shape or None, points of the exact grid that lie in several cells)
SHAPES = {"2d": ((37, 29), 825, (33, 33), 95), "3d": ((23, 19, 17), 5100, (17, 9, 9), 1265), "emix": ((23, 19, 17), 3025, None, None)}


@functools.lru_cache(maxsize=None)
def mesh_tuple(name):
    from knpemidg.mesh import make_mesh_2D, make_mesh_3D
    if name == "2d":
        return make_mesh_2D(0)
    if name == "3d":
        return make_mesh_3D(0, n_axons=4)
    from emix_sub import emix_submesh
    return emix_submesh()


def generic_bounds(mesh):
    d = mesh.gdim
    xmin, xmax = mesh.coords.min(axis=0), mesh.coords.max(axis=0)
    L = xmax - xmin
    return xmin - LO_FRAC[:d] * L, xmax + HI_FRAC[:d] * L


def exact_bounds(mesh):
    return mesh.coords.min(axis=0), mesh.coords.max(axis=0)


@functools.lru_cache(maxsize=None)
def spec(name, kind, tags=None):
    """kind "generic": the grid in generic position; "exact": from xmin to xmax, with points on facets, edges and vertices."""
    from knpemidg.grid import GridSpec
    mesh = mesh_tuple(name)[0]
    lo, hi = generic_bounds(mesh) if kind == "generic" else exact_bounds(mesh)
    return GridSpec(mesh.gdim, lo, hi, SHAPES[name][0] if kind == "generic" else SHAPES[name][2], tags=tags)


@functools.lru_cache(maxsize=None)
def located(name, kind):
    """(host owner, host lambda, locate_points' cells and lambda for the points that have an owner), computed once."""
    from knpemidg import recorder as R
    mesh = mesh_tuple(name)[0]
    s = spec(name, kind)
    owner, bary = s.locate(mesh)
    cells, lam = R.locate_points(mesh, s.points()[owner >= 0])
    return owner, bary, cells, lam


def candidate_pairs(mesh, pts, chunk=256):
    """(point index, cell index, lambda [n, d+1]) of every pair whose padded bounding box (locate_points' padding) holds the point."""
    X = mesh.coords[mesh.cells]
    lo, hi = X.min(axis=1), X.max(axis=1)
    pad = 1.0e-9 * (hi - lo).max(axis=1)[:, None]
    lo, hi = lo - pad, hi + pad
    T = (X[:, 1:, :] - X[:, :1, :]).transpose(0, 2, 1)
    pi, ci, lam = [], [], []
    for first in range(0, len(pts), chunk):
        p = pts[first:first + chunk]
        a, b = np.nonzero((p[:, None, 0] >= lo[None, :, 0]) & (p[:, None, 0] <= hi[None, :, 0]))      # axis by axis: few pairs survive x
        for k in range(1, mesh.gdim):
            keep = (p[a, k] >= lo[b, k]) & (p[a, k] <= hi[b, k])
            a, b = a[keep], b[keep]
        rhs = (p[a] - X[b, 0, :])[:, :, None]
        l = np.linalg.solve(T[b], rhs)[:, :, 0] if len(a) else np.zeros((0, mesh.gdim))
        pi.append(a + first)
        ci.append(b)
        lam.append(np.concatenate([1.0 - l.sum(axis=1, keepdims=True), l], axis=1))
    return np.concatenate(pi), np.concatenate(ci), np.concatenate(lam)


@functools.lru_cache(maxsize=None)
def candidates(name, kind):
    mesh = mesh_tuple(name)[0]
    return candidate_pairs(mesh, spec(name, kind).points())


def owners_from_candidates(npts, pi, ci, lam, tol=1.0e-12, allowed=None):
    """Lowest cell index among the accepted candidates of every point, -1 without one."""
    ok = lam.min(axis=1) >= -tol
    if allowed is not None:
        ok &= allowed[ci]
    owner = np.full(npts, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(owner, pi[ok], ci[ok])
    owner[owner == np.iinfo(np.int64).max] = -1
    return owner


def value_bound(mesh, pts, owner, u):
    """1e-11 kappa_i (1 + |p_i|_inf / diam_i) max_a |u[c_i, a]| per point (0 where owner is -1): a rounding bound for forming p - x0
    and solving for lambda in fp64, four orders above the machine epsilon; kappa_i = cond of the owning cell's edge matrix, diam_i
    its longest edge.  u [nc, nd]."""
    X = mesh.coords[mesh.cells]
    found = owner >= 0
    c = owner[found]
    T = (X[c, 1:, :] - X[c, :1, :]).transpose(0, 2, 1)
    kappa = np.linalg.cond(T)
    nv = X.shape[1]
    diam = np.max([np.linalg.norm(X[c, a] - X[c, b], axis=1) for a in range(nv) for b in range(a + 1, nv)], axis=0)
    out = np.zeros(len(owner))
    out[found] = 1.0e-11 * kappa * (1.0 + np.abs(pts[found]).max(axis=1) / diam) * np.abs(u[c]).max(axis=1)
    return out


def problem(name, p):
    """The oracle problem of a mesh with synthetic_state's discontinuous nodal values (a wrong owner shows)."""
    import knpemi_oracle as ko
    from common import synthetic_state
    m, s, f = mesh_tuple(name)
    if name == "emix":
        pb = ko.build_emix(m, s.array(), f.array(), p=p)
    else:
        pb = ko.build_idealized(m, s.array(), f.array(), p=p, membrane_tags=(1, 2) if name == "3d" else (1,))
    synthetic_state(pb, volt=1.0e3 if name == "emix" else 1.0)
    return pb


def nodal_fields(pb):
    """[phi, c_0 .. c_{n_sys-1}, c_elim], each [nc, nd], in field-id order."""
    nc = pb.mesh.num_cells()
    return [pb.phi.reshape(nc, -1)] + [c.reshape(nc, -1) for c in pb.c] + [pb.c_elim.reshape(nc, -1)]
