"""Meshes, selections and host references shared by tests/test_fieldmesh_host.py and tests/test_gpu_fieldmesh.py, at the smallest sizes
the project already uses: the cases of surface_cases.CASES (cell strides 3, 4, 6 and 10, the variable vertex valence of the EMIx
submesh, two membrane tags) with common.synthetic_state's nodal data, which are discontinuous from cell to cell, so a wrong cell or
dof shows.  Everything is computed once (lru_cache) and never changed.

Every case is taken with all cells and with the ECS alone (cell tag 0), continuous and not.  One combination has no output mesh: on
make_mesh_2D(0) the box that marks the cell cuts through the crossed cells, so every one of its 62 membrane facets lies between two
cells of tag 1, and the continuous output of all cells must be refused there (`refused`) -- the tests assert that refusal; the ECS of
that mesh and its discontinuous output have no such facet.

`brute` is an independent statement of the node values: a loop over the selected cells and their local dofs that names the mesh
entity by its vertex ids (a vertex id, or the pair of an edge's vertex ids -- no edge numbering) and accumulates per (entity, tag) in
extended precision.

The bound (`BOUND`): 2 * 2^-53 * sum_a |u_a| per value.  A sequential fp64 sum of m terms and one division err by at most
2^-53 sum_a |u_a| to first order in the mean (each of the m - 1 additions by 2^-53 of a partial sum, whose modulus is at most
sum |u_a|; divided by m the m - 1 errors add up to at most (m - 1) / m of that; the division adds 2^-53 |mean| <= 2^-53 sum |u_a| /
m); the bound is twice that."""
import functools

import numpy as np

from grid_cases import mesh_tuple, nodal_fields                 # noqa: F401  (shared caches)
from grid_cases import problem as _build_problem
from surface_cases import CASES, ion_names, membrane_tags       # noqa: F401

EPS = 2.0 ** -53
BOUND = 2.0 * EPS
ECS = (0,)
SELECTIONS = ("all", "ecs")
VTK_EDGES = {3: [(0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3)], 2: [(0, 1), (1, 2), (2, 0)]}
COMBOS = [(name, p, sel, cont) for name, p in CASES for sel in SELECTIONS for cont in (True, False)]


@functools.lru_cache(maxsize=None)
def problem(name, p):
    """grid_cases.problem, built once per case: nothing here changes it."""
    return _build_problem(name, p)


def refused(name, sel, continuous):
    """The combination whose continuous output would average across a membrane (see the head of the file)."""
    return name == "2d" and sel == "all" and continuous


def tags_of(sel):
    return None if sel == "all" else ECS


def stand_in_rank(nc, seed=5):
    """A fixed permutation standing in for _abi.Device.cell_rank where no device is at hand."""
    return np.random.default_rng(seed).permutation(nc).astype(np.int64)


def make_spec(name, p, sel="all", continuous=True, cell_rank=None, cell_tags=None, tags="by sel"):
    from knpemidg.fieldmesh import FieldMeshSpec
    mesh, sub, surf = mesh_tuple(name)
    return FieldMeshSpec(mesh, sub if cell_tags is None else cell_tags, surf, membrane_tags(name), p,
                         tags=tags_of(sel) if isinstance(tags, str) else tags, continuous=continuous, cell_rank=cell_rank)


@functools.lru_cache(maxsize=None)
def spec(name, p, sel="all", continuous=True, ranked=False):
    """The spec of a combination, numbered by (entity, tag) / (cell, dof), or -- ranked -- along stand_in_rank's cell order."""
    nc = mesh_tuple(name)[0].num_cells()
    return make_spec(name, p, sel, continuous, cell_rank=stand_in_rank(nc) if ranked else None)


def field_names(pb):
    return ["phi"] + ["c_" + k for k in ion_names(pb)]


def fields_of(pb):
    """{name: nodal values [nc, nd]} of phi and every concentration, the eliminated ion last."""
    return dict(zip(field_names(pb), nodal_fields(pb)))


def node_keys(s):
    """Per node of a spec the (entity, tag) key in brute's terms: the vertex id, or the pair of the edge's vertex ids."""
    ent = []
    for e in s.node_entity:
        ent.append(int(e) if e < s.n_vertices else tuple(int(v) for v in s.edge_vertices[e - s.n_vertices]))
    return list(zip(ent, (int(t) for t in s.node_tag)))


def one_cell_tags(name, cell):
    """The mesh's cell tags with `cell` alone carrying the new tag 7: tags=(7,) then selects that one cell."""
    ct = np.asarray(mesh_tuple(name)[1].array()).astype(np.int64).copy()
    ct[cell] = 7
    return ct


@functools.lru_cache(maxsize=None)
def brute(name, p, sel):
    """({(entity, tag): column}, mean [n_fields, n_keys], sum_a |u_a| [n_fields, n_keys], count [n_keys]) over the selected cells, in
    extended precision, fields in field_names order."""
    mesh, sub, surf = mesh_tuple(name)
    pb = problem(name, p)
    L = np.longdouble
    ct = np.asarray(sub.array()).astype(np.int64)
    U = np.stack([np.asarray(u, dtype=np.float64).reshape(mesh.num_cells(), -1) for u in nodal_fields(pb)])      # [nf, nc, nd]
    nv = mesh.gdim + 1
    pairs = [(a, b) for a in range(nv) for b in range(a + 1, nv)] if p == 2 else []
    col, entry_col, entry_cell, entry_dof = {}, [], [], []
    for c in range(mesh.num_cells()):
        if sel == "ecs" and int(ct[c]) not in ECS:
            continue
        v = [int(x) for x in mesh.cells[c]]
        ents = v + [tuple(sorted((v[a], v[b]))) for a, b in pairs]
        for a, e in enumerate(ents):
            k = col.setdefault((e, int(ct[c])), len(col))
            entry_col.append(k); entry_cell.append(c); entry_dof.append(a)
    entry_col, entry_cell, entry_dof = (np.asarray(x, dtype=np.int64) for x in (entry_col, entry_cell, entry_dof))
    vals = U[:, entry_cell, entry_dof].astype(L)                     # [nf, n_entries]
    total = np.zeros((len(U), len(col)), dtype=L)
    scale = np.zeros((len(U), len(col)), dtype=L)
    count = np.bincount(entry_col, minlength=len(col))
    for q in range(len(U)):
        np.add.at(total[q], entry_col, vals[q])
        np.add.at(scale[q], entry_col, np.abs(vals[q]))
    return col, total / count.astype(L), scale, count


def device_case(name, p):
    """(dev, pb): a context with the synthetic state of `problem`.  The caller closes dev."""
    from common import device_for, push_state
    pb = problem(name, p)
    dev = device_for(pb)
    push_state(dev, pb)
    return dev, pb


def device_frame(dev, pb, s, names=None, dtype=np.float64):
    """(handle, {field: array [n_nodes]}) of a sampler of the spec's lists, sampled once."""
    from knpemidg.fieldmesh import resolve_fields
    names = field_names(pb) if names is None else list(names)
    h = dev.fieldmesh_create(s.ptr, s.cell, s.dof, resolve_fields(names, ion_names(pb)), f32=np.dtype(dtype) == np.float32)
    dev.fieldmesh_sample(h)
    return h, dict(zip(names, dev.fieldmesh_fetch(h, len(names), s.n_nodes, dtype)))
