"""Meshes, selections and host references shared by tests/test_surface_host.py and tests/test_gpu_surface.py, at the smallest sizes
the project already uses: make_mesh_2D(0), make_mesh_3D(0, n_axons=4) (two membrane tags) and the EMIx submesh; the meshes and the
synthetic problems are those of grid_cases (one cache for both modules).  The nodal data are common.synthetic_state's: discontinuous
from cell to cell, so a swapped side or a wrong cell shows.

`brute_trace` is an independent statement of the facet mean of a one-sided trace: a loop over the facets that picks the side's cell
and local facet from mesh.facet_cells / mesh.facet_local, places a quadrature rule of knpemidg/quadrature.py that is exact for degree
2 on the facet and sums the nodal basis there, in extended precision -- its own rounding is far below the bound the tests hold the
project's float64 statement to.

The bound (`BOUND`): 8 eps sum_a |w_a u_a| per value.  The value is formed from at most 3 products (the weights), a sum of at most
3 terms and one division in fp64: each operation adds a relative error of at most eps = 2^-53 to terms whose moduli add up to
sum_a |w_a u_a|, 4 eps in all to first order; a factor 2 of margin."""
import functools

import numpy as np

from grid_cases import mesh_tuple, nodal_fields, problem        # noqa: F401  (shared caches)

EPS = 2.0 ** -53
BOUND = 8.0 * EPS
CASES = [("2d", 1), ("2d", 2), ("3d", 1), ("3d", 2), ("emix", 1)]


def membrane_tags(name):
    return (1, 2) if name in ("3d", "emix") else (1,)


@functools.lru_cache(maxsize=None)
def spec(name, p, tags=None):
    """Every membrane facet (tags None) or the facets of the given surface tags."""
    from knpemidg.surface import SurfaceSpec
    mesh, sub, surf = mesh_tuple(name)
    return SurfaceSpec(mesh, surf, sub, membrane_tags(name), degree=p, tags=tags)


def e_side(mesh, cell_tags, facets):
    """0 / 1: which entry of mesh.facet_cells is the `_e` cell (the side utils.plus gives: the lower tag, side 1 on equal tags)."""
    fc = mesh.facet_cells[facets]
    ct = np.asarray(cell_tags).astype(np.int64)
    return np.where(ct[fc[:, 0]] >= ct[fc[:, 1]], 1, 0)


def brute_trace(mesh, cell_tags, facets, u, degree, side):
    """(mean, sum_a |w_a u_a|) per facet of the trace of u [nc, nd] from side 0 (`_e`) / 1 (`_i`), facet by facet with a quadrature
    rule exact for degree 2, in extended precision."""
    from knpemidg.quadrature import simplex_rule
    from knpemidg.recorder import basis_weights
    d = mesh.gdim
    pts, w = simplex_rule(d - 1, 2)
    L = np.float128 if hasattr(np, "float128") else np.longdouble
    es = e_side(mesh, cell_tags, facets)
    u = np.asarray(u, dtype=np.float64).reshape(mesh.num_cells(), -1)
    mean, scale = np.empty(len(facets)), np.empty(len(facets))
    for i, f in enumerate(facets):
        s = es[i] if side == 0 else 1 - es[i]
        cell, lf = int(mesh.facet_cells[f, s]), int(mesh.facet_local[f, s])
        others = [a for a in range(d + 1) if a != lf]
        # the facet's vertices are the cell's vertices but the one opposite to it: check it against the facet table itself
        assert sorted(mesh.cells[cell][others]) == sorted(mesh.facets[f])
        lam = np.zeros((len(w), d + 1))
        lam[:, others] = pts
        B = basis_weights(lam, degree).astype(L)                      # [nq, nd]
        wa = (np.asarray(w, dtype=L)[:, None] * B).sum(axis=0)        # the exact weights of the nodal values, up to L's rounding
        ua = u[cell].astype(L)
        mean[i] = float((wa * ua).sum())
        scale[i] = float(np.abs(wa * ua).sum())
    return mean, scale


def facet_arrays(pb, seed=7):
    """Synthetic E [n_ions, nf] (the problem itself carries phi_M and I_ch only), phi_M [nf] and I_ch [n_ions, nf]."""
    nf = pb.mesh.num_facets()
    E = np.random.default_rng(seed).uniform(-0.1, 0.1, size=(len(pb.ions), nf))
    I = np.stack([pb.I_ch[ion["name"]] for ion in pb.ions])
    return pb.phi_M, E, I


def state_names(name):
    """The state planes of a case: n only mm_hh has (NaN on the facets of tag 2), V both models have."""
    return ["n", "V"] if len(membrane_tags(name)) == 2 else ["n"]


def device_case(name, p, tags=None, facets=None):
    """(dev, pb, spec, models, tables, E): a context with the synthetic state of `problem`, a synthetic E, mm_hh on the facets of tag
    1 and mm_leak on those of tag 2 with random state tables {handle: [rows, ns]}.  The caller closes dev."""
    from types import SimpleNamespace
    from common import device_for, push_state
    from knpemidg import _abi as A
    from knpemidg import recorder as R
    from knpemidg.models import mm_hh, mm_leak
    from knpemidg.surface import SurfaceSpec
    mesh, sub, surf = mesh_tuple(name)
    pb = problem(name, p)
    dev = device_for(pb)
    push_state(dev, pb)
    E = facet_arrays(pb)[1]
    dev.upload(A.F_E, E)
    rng = np.random.default_rng(11)
    models, tables = [], {}
    for tag, ode in zip(membrane_tags(name), (mm_hh, mm_leak)):
        f = R.membrane_facets(mesh, np.asarray(surf.array()), [tag])
        st = rng.uniform(-1.0, 1.0, size=(len(f), len(ode.init_state_values())))
        h = dev.ode_create(ode.MODEL_ID, f, st, np.tile(ode.init_parameter_values(), (len(f), 1)))
        models.append(SimpleNamespace(facets=f, ode=ode, handle=h, tag=tag))
        tables[h] = st
    s = spec(name, p) if tags is None and facets is None else SurfaceSpec(mesh, surf, sub, membrane_tags(name), degree=p, tags=tags,
                                                                           facets=facets)
    return dev, pb, s, models, tables, E


def device_frame(dev, pb, s, models, names, states, dtype=np.float64):
    """(handle, frame [planes, n]) of a sampler with the given field names and states, sampled once."""
    from knpemidg.surface import resolve_fields
    ids = resolve_fields(names, ion_names(pb))
    st = s.state_tables(models, states) if states else None
    h = dev.surf_create(s.facets, ids, states=st, f32=dtype == np.float32)
    dev.surf_sample(h)
    return h, dev.surf_fetch(h, len(names) + len(states), s.n, dtype)


def ion_names(pb):
    return [ion["name"] for ion in pb.ions]


def all_fields(pb):
    """Every field name of the problem's ions, in a fixed order."""
    ions = ion_names(pb)
    return (["phi_M"] + ["E_" + k for k in ions] + ["I_ch_" + k for k in ions] + ["I_ch_total", "phi_e", "phi_i"]
            + ["c_%s_e" % k for k in ions] + ["c_%s_i" % k for k in ions])
