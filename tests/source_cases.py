"""Inputs of the device-source tests (tests/test_expression_host.py checks their conditions, tests/test_gpu_source.py uses them).

For every mesh a box [a, b] and the source of tests/test_gpu_solver.py::test_f_source_array_and_callable_vs_oracle,

    f(x, t) = g * inside(a, b)(x) * (t0 <= t <= t1) * (1 + 0.3 sin(k x[0])),

once as the C++ string of a knpemidg.Expression and once as a hand-written numpy twin; the host rule (mms_terms._cell_source on the
twin) is the reference the device rows are compared with, and `scale` the per-entry magnitude vol * sum_q w_q |f(x_q)| |B[q][a]|
their difference is measured against."""
import functools

import numpy as np

G, T0, T1 = 40.0, 2.0e-4, 6.0e-4
T_IN, T_OUT = 3.0e-4, 0.0                # inside / outside the time window
# The box in fractions of the mesh extent, per axis (lower, upper).  The existing test's 0.2 .. 0.7 holds no whole ECS cell on the
# small boxes (their ECS is a one-cell rim around the ICS block), so the box is moved: it starts inside the mesh along x, below the
# mesh along the other axes (the rim cells touch the boundary), and ends inside the mesh along every axis.
BOX_FRACTION = ((0.05, 0.55), (-0.05, 0.55), (-0.05, 0.55))


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    """(mesh, subdomains, surfaces) of a case; built once per process."""
    from common import small_3d
    if name == "small_3d":
        return small_3d()
    if name == "small_3d_633":
        return small_3d((6, 3, 3))
    if name == "small_3d_844":
        return small_3d((8, 4, 4))
    if name == "mesh_2d":
        from knpemidg.mesh import make_mesh_2D
        return make_mesh_2D(0)
    if name == "emix_sub":
        from emix_sub import emix_submesh
        return emix_submesh()
    raise KeyError(name)


# (mesh, degree): the cases of the row-against-host-rule test
ROW_CASES = [("small_3d", 1), ("small_3d_633", 2), ("mesh_2d", 1), ("mesh_2d", 2), ("emix_sub", 1)]
MESHES = ["small_3d", "small_3d_633", "small_3d_844", "mesh_2d", "emix_sub"]


def box_of(mesh, fraction=BOX_FRACTION):
    lo, hi = mesh.coords.min(axis=0), mesh.coords.max(axis=0)
    fr = np.array(fraction[:mesh.gdim])
    return lo + fr[:, 0] * (hi - lo), lo + fr[:, 1] * (hi - lo)


def wavenumber(mesh):
    """k with k x[0] of order one over the mesh (4e5 / m on the micrometre boxes, as in the existing test)."""
    return 3.2 / float(np.abs(mesh.coords[:, 0]).max())


def code(dim):
    inside = " && ".join("x[%d] >= a%d && x[%d] <= b%d" % (d, d, d, d) for d in range(dim))
    return "g * ((%s) ? 1.0 : 0.0) * ((t0 <= t && t <= t1) ? 1.0 : 0.0) * (1.0 + 0.3 * sin(k * x[0]))" % inside


def params(mesh, t, g=G):
    """Keyword parameters of the Expression (t: a number or a Constant)."""
    a, b = box_of(mesh)
    out = dict(g=g, t0=T0, t1=T1, k=wavenumber(mesh), t=t)
    for d in range(mesh.gdim):
        out["a%d" % d], out["b%d" % d] = float(a[d]), float(b[d])
    return out


def expression(mesh, t, g=G):
    from knpemidg import Expression
    return Expression(code(mesh.gdim), degree=4, **params(mesh, t, g))


def twin(mesh, g=G):
    """The numpy twin f(X[..., dim], t)."""
    a, b = box_of(mesh)
    k = wavenumber(mesh)

    def f(X, t):
        inside = np.all((X >= a) & (X <= b), axis=-1)
        return g * inside * (T0 <= t) * (t <= T1) * (1.0 + 0.3 * np.sin(k * X[..., 0]))
    return f


def ecs_points(mesh, sub):
    """(ECS cells, X[cell, q, dim]) of the host rule."""
    from knpemidg.mms_terms import QDEG
    from knpemidg.quadrature import simplex_rule
    sel = np.nonzero(np.asarray(sub) == 0)[0]
    bary, _ = simplex_rule(mesh.gdim, QDEG)
    return sel, np.einsum("ql,cld->cqd", bary, mesh.coords[mesh.cells[sel]])


def host_row(mesh, sub, degree, f, t):
    """(row[nc, nd], scale[nc, nd]): the host rule on f(., t) over the cells with sub == 0, and the magnitude of each entry's sum."""
    from knpemidg.dgtab import tabulate
    from knpemidg.mms_terms import QDEG, _cell_source, _ev, _geometry
    from knpemidg.quadrature import simplex_rule
    vol = _geometry(mesh)[0]
    sel, X = ecs_points(mesh, sub)
    nd = tabulate(degree, simplex_rule(mesh.gdim, QDEG)[0])[0].shape[1]
    row = np.zeros((mesh.num_cells(), nd))
    _cell_source(mesh, vol, sel, lambda Y: f(Y, t), row, p=degree)
    bary, w = simplex_rule(mesh.gdim, QDEG)
    scale = np.zeros_like(row)
    scale[sel] = np.einsum("q,c,cq,qa->ca", w, vol[sel], np.abs(_ev(lambda Y: f(Y, t), X)), np.abs(tabulate(degree, bary)[0]))
    return row, scale


BOUND = 1.0e-12          # |device - host| <= BOUND * scale per entry: (125 + a few) roundings of 1.1e-16 ~ 2e-14, and a factor of ~50


def worst_ratio(got, row, scale):
    """max |got - row| / scale over the entries with scale > 0; entries with scale == 0 must be exact zeros (asserted here)."""
    got, row = np.asarray(got).reshape(row.shape), np.asarray(row)
    zero = scale == 0
    assert np.all(got[zero] == 0.0) and np.all(row[zero] == 0.0)
    return float((np.abs(got - row)[~zero] / scale[~zero]).max()) if (~zero).any() else 0.0
