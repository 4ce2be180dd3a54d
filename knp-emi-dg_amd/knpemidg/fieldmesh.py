"""Volume-field snapshots on the mesh itself (csrc/fieldmesh.hip): host side.

The traces, the voxel images and the membrane surface leave one thing out: phi and the concentrations on the mesh's own cells, where
the jump of phi across the membrane and an extracellular space a few cells thick can be seen.  `Solver.record_fields` samples them on
the device while the run goes on and writes `<name>.h5` plus an XDMF sidecar that ParaView opens.

Within one subdomain the DG solution is continuous up to the discretisation error, so a picture needs one value per (mesh entity,
cell tag): the arithmetic mean of the nodal values the selected cells of that tag have there.  An entity is a vertex (P1) or a
vertex or an edge (P2).  Cells of different tags never share a node: the membrane stays a jump.  `continuous=False` keeps the exact
DG values instead, one node per (cell, local dof).

`FieldMeshSpec` is the selection, the output mesh, the lists the kernel walks and the HOST statement of k_fieldmesh_sample
(`sample_host`): what runs without a device and what the tests compare the device with.  `FieldMeshFile` is the file; `FieldSampler`
is what `Solver.record_fields` returns.
"""
import os

import numpy as np

from knpemidg._abi import FM_C, FM_PHI, KnpError
from knpemidg.recorder import membrane_facets

MAX_SAMPLERS = 4           # KNP_FM_MAX (csrc/fieldmesh.hip)
# columns of the connectivity as the sidecar wants them (VTK's edge order; the project's is lexicographic: knp_set_tabulation), as
# positions among the edge columns.  tetrahedron: (0,1), (1,2), (0,2), (0,3), (1,3), (2,3); triangle: (0,1), (1,2), (2,0)
XDMF_EDGE_ORDER = {3: [0, 3, 1, 2, 4, 5], 2: [0, 2, 1]}
TOPOLOGY = {(2, 1): "Triangle", (3, 1): "Tetrahedron", (2, 2): "Triangle_6", (3, 2): "Tetrahedron_10"}


def resolve_fields(fields, ion_names):
    """(kind, ion) pairs of knp_fieldmesh_create for names out of "phi" and "c_<ion>" (ion_list order, the eliminated ion last), one
    per name in the order given.  ValueError naming the offender for an unknown or repeated name and an empty selection."""
    if isinstance(fields, str):
        fields = (fields,)
    ions = [str(n) for n in ion_names]
    table = {"phi": (FM_PHI, -1)}
    for k, ion in enumerate(ions):
        table["c_" + ion] = (FM_C, k)
    known = "phi, c_<ion> with <ion> out of " + ", ".join(ions)
    out, seen = [], []
    for f in fields:
        if not isinstance(f, str) or f not in table:
            raise ValueError("record_fields: unknown field %r (known: %s)" % (f, known))
        if f in seen:
            raise ValueError("record_fields: field %r is listed twice" % (f,))
        seen.append(f)
        out.append(table[f])
    if not out:
        raise ValueError("record_fields: no field to sample")
    return out


def local_edges(dim):
    """The vertex pairs (a, b), a < b, of the edge dofs in local order (knp_set_tabulation)."""
    nv = dim + 1
    return [(a, b) for a in range(nv) for b in range(a + 1, nv)]


class FieldMeshSpec:
    """The selected cells of a mesh (ascending caller's cell ids), the output nodes and the lists of the nodal values they average.

    mesh, cell_tags, facet_tags: the caller's mesh and tag arrays; membrane_tags: the surface tags the context treats as membrane.
    tags: the cell tags whose cells are written (default: every cell).  ValueError for an unknown or repeated tag, an empty selection
    and, with continuous=True, a membrane facet between two selected cells of the same tag (averaging would smear the membrane there).
    cell_rank [nc] (caller -> device cell order, _abi.Device.cell_rank): number the nodes along the device's cell order, so that
    consecutive nodes gather from nearby cells; without it they are numbered by (entity, tag), resp. (cell, dof).
      cells [n_sel], tag [n_sel]            the selected cells and their tags
      node_entity [n_nodes]                 vertex id, or n_vertices + edge id (edge ids: np.unique over the sorted vertex pairs of
                                            every cell of the mesh; `edge_vertices` [n_edges, 2])
      node_tag [n_nodes]                    the cell tag of the node
      points [n_nodes, 3]                   z = 0 in 2D; an edge node sits at the edge's midpoint
      connectivity [n_sel, nd]              nodes of every selected cell, local dof order (vertices, then the edges (a, b), a < b)
      ptr [n_nodes + 1], cell [nnz], dof [nnz]   CSR lists of the contributing (caller's cell, local dof) pairs, each list ascending
                                            by (cell, dof); with continuous=False every list has length one"""

    def __init__(self, mesh, cell_tags, facet_tags, membrane_tags, degree, tags=None, continuous=True, cell_rank=None):
        self.mesh, self.dim, self.degree, self.continuous = mesh, int(mesh.gdim), int(degree), bool(continuous)
        if self.degree not in (1, 2):
            raise ValueError("record_fields: degree must be 1 or 2")
        ct = np.asarray(cell_tags.array() if hasattr(cell_tags, "array") else cell_tags).astype(np.int64)
        ft = np.asarray(facet_tags.array() if hasattr(facet_tags, "array") else facet_tags).astype(np.int64)
        cells = np.asarray(mesh.cells).astype(np.int64)
        nc, nv = len(cells), self.dim + 1
        have = [int(t) for t in np.unique(ct)]
        if tags is None:
            want = have
        else:
            want = [int(t) for t in ([tags] if np.isscalar(tags) else tags)]
            for i, t in enumerate(want):
                if t in want[:i]:
                    raise ValueError("record_fields: tag %d is listed twice" % t)
                if t not in have:
                    raise ValueError("record_fields: tag %d is not a cell tag of the mesh (cell tags: %s)" % (t, have))
        sel = np.nonzero(np.isin(ct, want))[0]
        if not len(sel):
            raise ValueError("record_fields: the selection holds no cell (tags %s)" % (want,))
        if self.continuous:
            mf = membrane_facets(mesh, ft, [int(t) for t in membrane_tags])
            fc = np.asarray(mesh.facet_cells)[mf].astype(np.int64)
            smear = np.isin(ct[fc[:, 0]], want) & (ct[fc[:, 0]] == ct[fc[:, 1]])
            if smear.any():
                f = int(mf[smear][0])
                raise ValueError("record_fields: membrane facet %d separates two selected cells of tag %d: their mean would smear "
                                 "the membrane (continuous=False keeps the DG values)" % (f, int(ct[fc[smear][0, 0]])))
        self.cells = np.ascontiguousarray(sel, dtype=np.int64)
        self.tag = ct[sel]
        self.n_sel = len(sel)
        # ---- the entity of every (cell, local dof): vertices, then edges
        n_vertices = len(mesh.coords)
        ent = [cells]
        self.edge_vertices = np.zeros((0, 2), dtype=np.int64)
        if self.degree == 2:
            le = local_edges(self.dim)
            pairs = np.stack([cells[:, [a, b]] for a, b in le], axis=1)               # [nc, ne, 2], ascending inside (cells are)
            self.edge_vertices, eid = np.unique(pairs.reshape(-1, 2), axis=0, return_inverse=True)
            ent.append(n_vertices + eid.reshape(nc, len(le)))
        ent = np.concatenate(ent, axis=1)[sel]                                        # [n_sel, nd]
        self.nd = nd = ent.shape[1]
        self.n_vertices = n_vertices
        e_cell = np.repeat(sel, nd)
        e_dof = np.tile(np.arange(nd, dtype=np.int64), self.n_sel)
        e_ent = ent.ravel()
        e_tag = np.repeat(self.tag, nd)
        rank = np.arange(nc, dtype=np.int64) if cell_rank is None else np.asarray(cell_rank, dtype=np.int64)
        if rank.shape != (nc,):
            raise ValueError("record_fields: cell_rank must hold one entry per cell")
        if self.continuous:
            # a node per (entity, tag); numbered by the lowest device cell that touches it, then by (entity, tag)
            ti = np.searchsorted(np.asarray(have), e_tag)
            key = e_ent * len(have) + ti
            ukey, inv = np.unique(key, return_inverse=True)
            if cell_rank is not None:
                first = np.full(len(ukey), nc, dtype=np.int64)
                np.minimum.at(first, inv, rank[e_cell])
                order = np.lexsort((ukey, first))
                new = np.empty(len(ukey), dtype=np.int64)
                new[order] = np.arange(len(ukey))
                inv = new[inv]
        else:
            # a node per (cell, dof), cells in device order
            pos = np.empty(self.n_sel, dtype=np.int64)
            pos[np.argsort(rank[sel], kind="stable")] = np.arange(self.n_sel)
            inv = np.repeat(pos, nd) * nd + e_dof
        self.n_nodes = n_nodes = int(inv.max()) + 1
        by = np.lexsort((e_dof, e_cell, inv))                                          # by node, then (cell, dof)
        self.cell = np.ascontiguousarray(e_cell[by])
        self.dof = np.ascontiguousarray(e_dof[by])
        self.ptr = np.zeros(n_nodes + 1, dtype=np.int64)
        np.cumsum(np.bincount(inv, minlength=n_nodes), out=self.ptr[1:])
        self.node_entity = np.empty(n_nodes, dtype=np.int64)
        self.node_tag = np.empty(n_nodes, dtype=np.int64)
        self.node_entity[inv] = e_ent
        self.node_tag[inv] = e_tag
        self.connectivity = np.ascontiguousarray(inv.reshape(self.n_sel, nd))
        coords = np.asarray(mesh.coords, dtype=np.float64)
        self.points = np.zeros((n_nodes, 3))
        is_v = self.node_entity < n_vertices
        self.points[is_v, :self.dim] = coords[self.node_entity[is_v]]
        if (~is_v).any():
            ev = self.edge_vertices[self.node_entity[~is_v] - n_vertices]
            self.points[~is_v, :self.dim] = 0.5 * (coords[ev[:, 0]] + coords[ev[:, 1]])

    def xdmf_connectivity(self):
        """connectivity with the edge columns in the order the sidecar's quadratic topology types want (XDMF_EDGE_ORDER)."""
        if self.degree == 1:
            return self.connectivity
        nv = self.dim + 1
        cols = list(range(nv)) + [nv + e for e in XDMF_EDGE_ORDER[self.dim]]
        return np.ascontiguousarray(self.connectivity[:, cols])

    def sample_host(self, fields, dtype=np.float64):
        """The host statement of k_fieldmesh_sample.  fields: {name: nodal values [nc, nd]} in the caller's cell order; returns {name:
        array [n_nodes]}.  Per node the first listed value, the further ones added one by one in list order, then ONE division by
        the list's length, in fp64; dtype float32 rounds that value once."""
        length = np.diff(self.ptr)
        out = {}
        nc = len(self.mesh.cells)
        for name, u in fields.items():
            u = np.asarray(u, dtype=np.float64).reshape(nc, -1)
            if u.shape[1] != self.nd:
                raise ValueError("fieldmesh: the nodal field holds %d values per cell, degree %d has %d" % (u.shape[1], self.degree, self.nd))
            s = u[self.cell[self.ptr[:-1]], self.dof[self.ptr[:-1]]].copy()
            for j in range(1, int(length.max())):
                more = np.nonzero(length > j)[0]
                at = self.ptr[more] + j
                s[more] = s[more] + u[self.cell[at], self.dof[at]]
            out[name] = (s / length.astype(np.float64)).astype(dtype)
        return out


# ---------------------------------------------------------------------------------------------------- files
def _xdmf_text(h5_name, spec, fields, times, precision):
    n, nn, nd = spec.n_sel, spec.n_nodes, spec.nd
    topo = '<Topology TopologyType="%s" NumberOfElements="%d">' % (TOPOLOGY[(spec.dim, spec.degree)], n)
    out = ['<?xml version="1.0" ?>', '<Xdmf Version="3.0">', ' <Domain>',
           '  <Grid Name="%s" GridType="Collection" CollectionType="Temporal">' % os.path.splitext(h5_name)[0]]
    for k, t in enumerate(times):
        out += ['   <Grid Name="frame_%d" GridType="Uniform">' % k,
                '    <Time Value="%r"/>' % float(t),
                '    ' + topo,
                '     <DataItem Format="HDF" NumberType="Int" Precision="8" Dimensions="%d %d">%s:/mesh/connectivity</DataItem>'
                % (n, nd, h5_name),
                '    </Topology>',
                '    <Geometry GeometryType="XYZ">',
                '     <DataItem Format="HDF" NumberType="Float" Precision="8" Dimensions="%d 3">%s:/mesh/points</DataItem>' % (nn, h5_name),
                '    </Geometry>',
                '    <Attribute Name="tag" AttributeType="Scalar" Center="Cell">',
                '     <DataItem Format="HDF" NumberType="Int" Precision="8" Dimensions="%d">%s:/mesh/tag</DataItem>' % (n, h5_name),
                '    </Attribute>']
        for f in fields:
            out += ['    <Attribute Name="%s" AttributeType="Scalar" Center="Node">' % f,
                    '     <DataItem Format="HDF" NumberType="Float" Precision="%d" Dimensions="%d">%s:/%s/vector_%d</DataItem>'
                    % (precision, nn, h5_name, f, k),
                    '    </Attribute>']
        out.append('   </Grid>')
    out += ['  </Grid>', ' </Domain>', '</Xdmf>', '']
    return "\n".join(out)


class FieldMeshFile:
    """`path` (.h5) with /mesh/{points, connectivity, cells, tag, node_entity, node_tag}, /t, /step and /<field>/vector_<k>
    ([n_nodes], one per frame), streamed through h5lite.H5Writer under a temporary name and renamed by close(), which also writes the
    XDMF sidecar next to it: a temporal collection whose frames share one Topology (Triangle, Tetrahedron, Triangle_6, Tetrahedron_10)
    and one XYZ Geometry and carry every field as a Scalar attribute centred on the nodes, plus the cell tag centred on the cells.
    /mesh/connectivity is what the sidecar reads: for P2 its edge columns are in VTK's order (FieldMeshSpec.xdmf_connectivity)."""

    def __init__(self, path, spec, fields, step_offset=0, precision=4):
        from knpemidg.h5lite import H5Writer
        self.path = os.fspath(path)
        folder = os.path.dirname(os.path.abspath(self.path))
        os.makedirs(folder, exist_ok=True)
        self.tmp = os.path.join(folder, ".%s.tmp%d" % (os.path.basename(self.path), os.getpid()))
        self.spec, self.fields = spec, list(fields)
        self.t, self.step = [], []
        self.precision = int(precision)
        w = self.w = H5Writer(self.tmp)
        w.write("/mesh/points", spec.points)
        w.write("/mesh/connectivity", spec.xdmf_connectivity().astype(np.int64))
        w.write("/mesh/cells", spec.cells.astype(np.int64))
        w.write("/mesh/tag", spec.tag.astype(np.int64))
        w.write("/mesh/node_entity", spec.node_entity.astype(np.int64))
        w.write("/mesh/node_tag", spec.node_tag.astype(np.int64))
        if step_offset:
            w.write("/step_offset", np.asarray([int(step_offset)], dtype=np.int64))

    def add(self, t, step, frame):
        k = len(self.t)
        for f in self.fields:
            a = np.asarray(frame[f])
            if a.shape != (self.spec.n_nodes,):
                raise ValueError("field-mesh file: field %r must hold one value per node" % f)
            self.precision = a.dtype.itemsize
            self.w.write("/%s/vector_%d" % (f, k), a)
        self.t.append(float(t))
        self.step.append(int(step))

    def abandon(self):
        """Drop the temporary file: nothing appears under the final name."""
        if self.w is not None and self.w.fh is not None:
            self.w.fh.close()
        self.w = None
        if os.path.exists(self.tmp):
            os.remove(self.tmp)

    def __del__(self):
        try:
            self.abandon()
        except Exception:
            pass

    def close(self):
        if self.w is None:
            return self.path
        try:
            self.w.write("/t", np.asarray(self.t, dtype=np.float64))
            self.w.write("/step", np.asarray(self.step, dtype=np.int64))
            self.w.close()
            self.w = None
            os.replace(self.tmp, self.path)
        finally:
            self.abandon()
        xdmf = os.path.splitext(self.path)[0] + ".xdmf"
        with open(xdmf + ".tmp%d" % os.getpid(), "w") as fh:
            fh.write(_xdmf_text(os.path.basename(self.path), self.spec, self.fields, self.t, self.precision))
        os.replace(xdmf + ".tmp%d" % os.getpid(), xdmf)
        return self.path


# ---------------------------------------------------------------------------------------------------- device
class FieldSampler:
    """One field-mesh sampler on the device (`Solver.record_fields`).  sample() returns {field: array [n_nodes]}; `points`,
    `connectivity`, `node_entity`, `node_tag`, `cells` describe the output mesh (FieldMeshSpec); field_ids as resolve_fields gives
    them.  make_spec(membrane_tags, cell_rank) builds the FieldMeshSpec once the device context exists."""

    def __init__(self, make_spec, fields, field_ids, every=1, dtype=np.float32, name="fields"):
        self.fields, self.field_ids = list(fields), list(field_ids)
        self.every = int(every)
        if self.every < 1:
            raise ValueError("record_fields: every must be a positive number of steps")
        try:
            self.dtype = np.dtype(dtype)
        except TypeError:
            raise ValueError("record_fields: dtype must be float64 or float32")
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("record_fields: dtype must be float64 or float32")
        self.name = str(name)
        if not self.name or os.sep in self.name or "/" in self.name:
            raise ValueError("record_fields: name must be a plain file stem")
        self._make_spec, self.spec = make_spec, None
        self.dev = self.handle = None
        self._file = None
        self._waiting = []              # (t, step) of the frames enqueued on the device and not yet written
        self._scratch = None

    @property
    def attached(self):
        return self.dev is not None and self.handle is not None

    def attach(self, dev, membrane_tags):
        if self.spec is None:
            self.spec = self._make_spec(membrane_tags, dev.cell_rank)
        s = self.spec
        self.handle = dev.fieldmesh_create(s.ptr, s.cell, s.dof, self.field_ids, f32=self.dtype == np.float32)
        self.dev = dev

    def _need_spec(self):
        if self.spec is None:
            raise KnpError("the field-mesh sampler is not on a device context yet (its nodes are numbered along the device's cell order)")
        return self.spec

    points = property(lambda self: self._need_spec().points)
    connectivity = property(lambda self: self._need_spec().connectivity)
    node_entity = property(lambda self: self._need_spec().node_entity)
    node_tag = property(lambda self: self._need_spec().node_tag)
    cells = property(lambda self: self._need_spec().cells)

    def _need_device(self):
        if not self.attached:
            raise KnpError("the field-mesh sampler is not on a device context yet")

    def _fetch(self, out=None):
        a = self.dev.fieldmesh_fetch(self.handle, len(self.fields), self.spec.n_nodes, self.dtype, out=out)
        return {f: a[q] for q, f in enumerate(self.fields)}

    def sample(self):
        """The fields as they are now (waits for this frame).  Not between the frames of a running time loop's file."""
        self._need_device()
        if self._waiting:
            raise KnpError("FieldSampler.sample: frames of the time loop's file are still waiting")
        self.dev.fieldmesh_sample(self.handle)
        return self._fetch()

    def timing(self):
        """dict(sample_ms, copy_ms): kernel and copy of the last fetched frame, from HIP events."""
        self._need_device()
        return dict(zip(("sample_ms", "copy_ms"), self.dev.fieldmesh_timing(self.handle)))

    # -- the time loops' file ---------------------------------------------------------------------------------------------------
    def begin(self, filename, k0, t):
        """Open `<filename><name>[_from<k0>].h5` and enqueue frame 0: the state the loop starts from."""
        self._need_device()
        part = "_from%d" % k0 if k0 else ""
        self._file = FieldMeshFile(filename + self.name + part + ".h5", self.spec, self.fields, step_offset=k0, precision=self.dtype.itemsize)
        self._enqueue(t, k0)

    def _enqueue(self, t, step):
        if self._waiting:
            self._write_one()           # frame n goes to the file while the steps queued after it run
        self.dev.fieldmesh_sample(self.handle)
        self._waiting.append((float(t), int(step)))

    def _write_one(self):
        t, step = self._waiting.pop(0)
        if self._scratch is None:       # the file takes the values at once: one buffer serves every frame of the loop
            self._scratch = np.empty((len(self.fields), self.spec.n_nodes), dtype=self.dtype)
        self._file.add(t, step, self._fetch(self._scratch))

    def after_step(self, steps_done, t):
        if self._file is not None and steps_done % self.every == 0:
            self._enqueue(t, steps_done)

    def finish(self):
        """Write the waiting frames, close the file and write the sidecar.  When a waiting frame cannot be fetched (the loop ended
        in a device error) the file is closed with the frames it has and the error goes on."""
        if self._file is None:
            return None
        try:
            while self._waiting:
                self._write_one()
        finally:
            f, self._file = self._file, None
            self._scratch = None
            path = f.close()
        return path

    def close(self):
        if self.attached and getattr(self.dev, "ctx", None):
            self.dev.fieldmesh_destroy(self.handle)
        self.dev = self.handle = None
