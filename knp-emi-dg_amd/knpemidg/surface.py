"""Membrane-surface snapshots (csrc/surface.hip): host side.

An EMI run exists to show what happens ON the membrane: the action potential travelling along an axon, [K+] piling up outside it,
the patch of an astrocyte that carries current.  The recorder gives set means, the voxel grid images the volume; here
`Solver.record_membrane` samples, per membrane facet, phi_M, the Nernst potentials, the channel currents, the one-sided traces of phi
and the concentrations and gating variables on the device while the run goes on, and writes them as cell data of a triangle
(3D) / segment (2D) surface mesh: `<name>.h5` plus an XDMF sidecar that ParaView opens.

`SurfaceSpec` is the selection, the surface mesh and the HOST statement of k_surf_sample (`sample_host`): what runs without a device and
what the tests compare the device with.  `SurfaceFile` is the file; `MembraneSampler` is what `Solver.record_membrane` returns.

Sides: `_e` is the cell the interface normal n_g leaves (utils.plus: the lower subdomain tag, row entry cell_e of the device's
membrane-facet table), `_i` the one it ends in (utils.minus).  The connectivity orders every facet's vertices so that its normal
points from the `_i` cell to the `_e` cell.
"""
import os

import numpy as np

from knpemidg._abi import SF_E, SF_I_CH, SF_I_CH_TOTAL, SF_PHI_M, SF_TRACE_E, SF_TRACE_I, KnpError
from knpemidg.recorder import facet_areas, membrane_facets, model_has_state

MAX_PLANES = 48            # KNP_SURF_MAX_PLANES (csrc/surface.hip)
MAX_SAMPLERS = 4           # KNP_SURF_MAX
_RESERVED_IONS = ("total",)     # "I_ch_total" is the sum over the ions


def resolve_fields(fields, ion_names):
    """(kind, ion) pairs of knp_surf_create for names out of "phi_M", "E_<ion>", "I_ch_<ion>", "I_ch_total", "phi_e", "phi_i",
    "c_<ion>_e" and "c_<ion>_i" (ion_list order, the eliminated ion last; ion -1 stands for phi), one per name in the order given.
    ValueError naming the offender for an unknown or repeated name, an empty selection and an ion whose name collides with a
    reserved one."""
    if isinstance(fields, str):
        fields = (fields,)
    ions = [str(n) for n in ion_names]
    for reserved in _RESERVED_IONS:
        if reserved in ions:
            raise ValueError("record_membrane: an ion named %r cannot be told from the reserved name 'I_ch_%s'" % (reserved, reserved))
    table = {"phi_M": (SF_PHI_M, -1), "I_ch_total": (SF_I_CH_TOTAL, -1), "phi_e": (SF_TRACE_E, -1), "phi_i": (SF_TRACE_I, -1)}
    for k, ion in enumerate(ions):
        table["E_" + ion] = (SF_E, k)
        table["I_ch_" + ion] = (SF_I_CH, k)
        table["c_%s_e" % ion] = (SF_TRACE_E, k)
        table["c_%s_i" % ion] = (SF_TRACE_I, k)
    known = "phi_M, E_<ion>, I_ch_<ion>, I_ch_total, phi_e, phi_i, c_<ion>_e, c_<ion>_i with <ion> out of " + ", ".join(ions)
    out, seen = [], []
    for f in fields:
        if not isinstance(f, str) or f not in table:
            raise ValueError("record_membrane: unknown field %r (known: %s)" % (f, known))
        if f in seen:
            raise ValueError("record_membrane: field %r is listed twice" % (f,))
        seen.append(f)
        out.append(table[f])
    if not out:
        raise ValueError("record_membrane: no field to sample")
    return out


def check_names(fields, states):
    """The plane names of a sampler: fields, then states.  ValueError for a repeated state, a state named like a field, no plane at
    all or more than MAX_PLANES."""
    fields, states = list(fields), [str(s) for s in states]
    for i, s in enumerate(states):
        if s in states[:i]:
            raise ValueError("record_membrane: state %r is listed twice" % s)
        if s in fields:
            raise ValueError("record_membrane: state %r has the name of a field" % s)
    if not fields and not states:
        raise ValueError("record_membrane: no field and no state to sample")
    if len(fields) + len(states) > MAX_PLANES:
        raise ValueError("record_membrane: at most %d field and state planes" % MAX_PLANES)
    return fields + states


def trace_weights(dim, degree):
    """w [dim + 1][nd]: w[l] are the weights of a cell's nodal values in the mean of their trace over local facet l (the facet
    opposite to vertex l), in the local dof order of knp_set_tabulation (vertices, then the edges (a, b), a < b).  P1: 1 / dim on
    the facet's vertices; P2: the exact mean of the quadratic -- in 2D (1, 4, 1) / 6 on the two vertices and the edge between them
    (Simpson), in 3D 1 / 3 on the three edges of the facet and 0 on its vertices."""
    nv = dim + 1
    edges = [(a, b) for a in range(nv) for b in range(a + 1, nv)]
    if degree == 1:
        w = np.full((nv, nv), 1.0 / dim)
        w[np.arange(nv), np.arange(nv)] = 0.0
        return w
    if degree != 2:
        raise ValueError("degree must be 1 or 2")
    w = np.zeros((nv, nv + len(edges)))
    for l in range(nv):
        for a in range(nv):
            if a != l and dim == 2:
                w[l, a] = 1.0 / 6.0
        for e, (a, b) in enumerate(edges):
            if a != l and b != l:
                w[l, nv + e] = 4.0 / 6.0 if dim == 2 else 1.0 / 3.0
    return w


class SurfaceSpec:
    """The selected membrane facets of a mesh (ascending caller's facet ids) and their surface mesh.

    mesh, facet_tags, cell_tags: the caller's mesh and tag arrays; membrane_tags: the surface tags the context treats as membrane
    (recorder.membrane_facets classifies).  tags: surface tags to select (default: every membrane tag); facets: explicit facet
    ids instead -- the two are mutually exclusive.  ValueError for a facet that is not a membrane facet, a repeated one, an unknown
    tag and an empty selection.
      facets [n], tags [n], cells [n, 2] (the `_e` and `_i` cell), local [n, 2] (their local facets), area [n]
      points [nv, 3] (only the vertices the selection uses, z = 0 in 2D), connectivity [n, 3] / [n, 2] into points"""

    def __init__(self, mesh, facet_tags, cell_tags, membrane_tags, degree=1, tags=None, facets=None):
        self.mesh, self.dim, self.degree = mesh, int(mesh.gdim), int(degree)
        ft = np.asarray(facet_tags.array() if hasattr(facet_tags, "array") else facet_tags).astype(np.int64)
        ct = np.asarray(cell_tags.array() if hasattr(cell_tags, "array") else cell_tags).astype(np.int64)
        mtags = [int(t) for t in membrane_tags]
        if tags is not None and facets is not None:
            raise ValueError("record_membrane: tags and facets are mutually exclusive")
        allmf = membrane_facets(mesh, ft, mtags)
        if facets is not None:
            try:
                sel = np.asarray(list(facets))
            except TypeError:
                raise ValueError("record_membrane: facets must be a sequence of facet ids")
            if sel.ndim != 1 or (len(sel) and sel.dtype.kind not in "iu"):
                raise ValueError("record_membrane: facets must be a sequence of whole facet ids")
            sel = sel.astype(np.int64)
            if not len(sel):
                raise ValueError("record_membrane: the selection holds no facet")
            uniq, counts = np.unique(sel, return_counts=True)
            if (counts > 1).any():
                raise ValueError("record_membrane: facet %d is listed twice" % int(uniq[counts > 1][0]))
            bad = uniq[~np.isin(uniq, allmf)]
            if len(bad):
                raise ValueError("record_membrane: facet %d is not a membrane facet" % int(bad[0]))
            sel = uniq
        else:
            want = mtags if tags is None else [int(t) for t in ([tags] if np.isscalar(tags) else tags)]
            for i, t in enumerate(want):
                if t in want[:i]:
                    raise ValueError("record_membrane: tag %d is listed twice" % t)
                if t not in mtags:
                    raise ValueError("record_membrane: tag %d is not a membrane tag (membrane tags: %s)" % (t, mtags))
            sel = allmf[np.isin(ft[allmf], want)]
            if not len(sel):
                raise ValueError("record_membrane: the selection holds no facet (tags %s)" % (want,))
        self.facets = np.ascontiguousarray(sel, dtype=np.int64)
        self.n = len(sel)
        self.tags = ft[sel]
        fc = np.asarray(mesh.facet_cells)[sel].astype(np.int64)
        fl = np.asarray(mesh.facet_local)[sel].astype(np.int64)
        # the side n_g leaves: the lower cell tag, side 1 on equal tags (utils.InterfaceNormal, context_tables.hpp)
        e_side = np.where(ct[fc[:, 0]] >= ct[fc[:, 1]], 1, 0)
        rows = np.arange(self.n)
        self.cells = np.stack([fc[rows, e_side], fc[rows, 1 - e_side]], axis=1)
        self.local = np.stack([fl[rows, e_side], fl[rows, 1 - e_side]], axis=1)
        self.area = facet_areas(mesh, sel)
        # ---- the surface mesh: vertices of every facet ordered so that the normal points from the _i cell to the _e cell
        coords = np.asarray(mesh.coords, dtype=np.float64)
        fv = np.asarray(mesh.facets)[sel].astype(np.int64)
        X = coords[fv]
        centre = coords[np.asarray(mesh.cells)[self.cells]].mean(axis=2)       # [n, 2, d]
        out = centre[:, 0] - centre[:, 1]
        if self.dim == 3:
            nrm = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        else:
            t = X[:, 1] - X[:, 0]
            nrm = np.stack([t[:, 1], -t[:, 0]], axis=1)                        # the segment direction turned 90 degrees clockwise
        flip = np.einsum("nd,nd->n", nrm, out) < 0.0
        fv[flip] = fv[flip][:, ::-1] if self.dim == 2 else fv[flip][:, [0, 2, 1]]
        used = np.unique(fv)
        self.vertices = used                                                    # caller's vertex ids of the rows of points
        self.points = np.zeros((len(used), 3))
        self.points[:, :self.dim] = coords[used]
        self.connectivity = np.searchsorted(used, fv).astype(np.int64)
        self._w = trace_weights(self.dim, self.degree)

    def normals(self):
        """[n, 3] the (not normalised) normal the vertex order of every facet defines: right-hand in 3D, the segment direction
        turned 90 degrees clockwise in 2D."""
        X = self.points[self.connectivity]
        if self.dim == 3:
            return np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        t = X[:, 1] - X[:, 0]
        return np.stack([t[:, 1], -t[:, 0], np.zeros(self.n)], axis=1)

    def trace(self, u, side):
        """(mean [n], scale [n]) of the trace of the nodal field u [nc, nd] (caller's cell order) from side 0 (`_e`) or 1 (`_i`)
        over every selected facet, with k_surf_sample's arithmetic: the facet's dofs in ascending local order, summed one by
        one (in 2D P2 the edge value times 4), then one division by dim (P1), 3 (P2, 3D) or 6 (P2, 2D).  scale = sum_a |w_a u_a|,
        what a rounding bound for the mean is proportional to."""
        d, nv = self.dim, self.dim + 1
        u = np.asarray(u, dtype=np.float64).reshape(len(self.mesh.cells), -1)
        if u.shape[1] != self._w.shape[1]:
            raise ValueError("surface: the nodal field holds %d values per cell, degree %d has %d" % (u.shape[1], self.degree, self._w.shape[1]))
        v = u[self.cells[:, side]]
        lf = self.local[:, side]
        s = np.zeros(self.n)
        if self.degree == 1 or d == 2:
            for a in range(nv):
                s = s + np.where(a != lf, v[:, a], 0.0)
        if self.degree == 2:
            e = nv
            for a in range(nv):
                for b in range(a + 1, nv):
                    ve = 4.0 * v[:, e] if d == 2 else v[:, e]
                    s = s + np.where((a != lf) & (b != lf), ve, 0.0)
                    e += 1
        div = float(d) if self.degree == 1 else (3.0 if d == 3 else 6.0)
        return s / div, (np.abs(self._w[lf]) * np.abs(v)).sum(axis=1)

    def sample_host(self, fields, phi_M=None, E=None, I_ch=None, phi=None, conc=None, states=None, state_tables=None):
        """The host statement of k_surf_sample: {plane: array [n]}.  fields: (name, (kind, ion)) pairs, the second as resolve_fields
        gives them.  phi_M [nf]; E, I_ch [n_ions, nf]; phi [nc, nd]; conc [n_ions][nc, nd] (the eliminated ion last), in the
        caller's numbering.  states: (name, handle [n], row [n], col [n]) per state plane, state_tables: {handle: table [rows, ns]};
        handle -1 gives NaN."""
        out = {}
        f = self.facets
        for name, (kind, ion) in fields:
            if kind == SF_PHI_M:
                v = np.asarray(phi_M, dtype=np.float64)[f]
            elif kind == SF_E:
                v = np.asarray(E, dtype=np.float64)[ion][f]
            elif kind == SF_I_CH:
                v = np.asarray(I_ch, dtype=np.float64)[ion][f]
            elif kind == SF_I_CH_TOTAL:
                I = np.asarray(I_ch, dtype=np.float64)
                v = I[0][f].copy()
                for k in range(1, len(I)):
                    v = v + I[k][f]
            elif kind in (SF_TRACE_E, SF_TRACE_I):
                v = self.trace(phi if ion < 0 else conc[ion], 0 if kind == SF_TRACE_E else 1)[0]
            else:
                raise ValueError("surface: unknown kind %r" % (kind,))
            out[name] = np.array(v, dtype=np.float64)
        for name, handle, row, col in states or ():
            v = np.full(self.n, np.nan)
            handle = np.asarray(handle)
            for h in np.unique(handle[handle >= 0]):
                m = handle == h
                v[m] = np.asarray(state_tables[int(h)], dtype=np.float64)[np.asarray(row)[m], np.asarray(col)[m]]
            out[name] = v
        return out

    def state_tables(self, models, names):
        """(handle, row, col), each [len(names), n], of knp_surf_create.  models: the membrane models -- anything with `facets`
        (row r of the state table belongs to facets[r]), `ode.state_indices(name)` and `handle`.  A facet whose model has no state
        of that name gets handle -1; ValueError naming the state when no selected facet has it."""
        names = list(names)
        handle = np.full((len(names), self.n), -1, dtype=np.int32)
        row = np.zeros((len(names), self.n), dtype=np.int64)
        col = np.zeros((len(names), self.n), dtype=np.int32)
        for m in models:
            if getattr(m, "handle", None) is None:             # a model that lives on the host has no device table
                continue
            mf = np.asarray(m.facets, dtype=np.int64)
            order = np.argsort(mf, kind="stable")
            pos = np.searchsorted(mf[order], self.facets)
            ok = pos < len(mf)
            ok[ok] = mf[order][pos[ok]] == self.facets[ok]
            for q, name in enumerate(names):
                if not model_has_state(m.ode, name):
                    continue
                handle[q, ok] = int(m.handle)
                row[q, ok] = order[pos[ok]]
                col[q, ok] = int(m.ode.state_indices(name))
        for q, name in enumerate(names):
            if not (handle[q] >= 0).any():
                raise ValueError("record_membrane: no selected facet belongs to a membrane model with a state '%s'" % name)
        return handle, row, col


# ---------------------------------------------------------------------------------------------------- files
def _xdmf_text(h5_name, spec, planes, times, precision):
    n, nv = spec.n, len(spec.points)
    topo = ('<Topology TopologyType="Triangle" NumberOfElements="%d">' % n if spec.dim == 3 else
            '<Topology TopologyType="Polyline" NodesPerElement="2" NumberOfElements="%d">' % n)
    out = ['<?xml version="1.0" ?>', '<Xdmf Version="3.0">', ' <Domain>',
           '  <Grid Name="%s" GridType="Collection" CollectionType="Temporal">' % os.path.splitext(h5_name)[0]]
    for k, t in enumerate(times):
        out += ['   <Grid Name="frame_%d" GridType="Uniform">' % k,
                '    <Time Value="%r"/>' % float(t),
                '    ' + topo,
                '     <DataItem Format="HDF" NumberType="Int" Precision="8" Dimensions="%d %d">%s:/surface/connectivity</DataItem>'
                % (n, spec.dim, h5_name),
                '    </Topology>',
                '    <Geometry GeometryType="XYZ">',
                '     <DataItem Format="HDF" NumberType="Float" Precision="8" Dimensions="%d 3">%s:/surface/points</DataItem>' % (nv, h5_name),
                '    </Geometry>']
        for f in planes:
            out += ['    <Attribute Name="%s" AttributeType="Scalar" Center="Cell">' % f,
                    '     <DataItem Format="HDF" NumberType="Float" Precision="%d" Dimensions="%d">%s:/%s/vector_%d</DataItem>'
                    % (precision, n, h5_name, f, k),
                    '    </Attribute>']
        out.append('   </Grid>')
    out += ['  </Grid>', ' </Domain>', '</Xdmf>', '']
    return "\n".join(out)


class SurfaceFile:
    """`path` (.h5) with /surface/{points, connectivity, facet, tag, cells, area}, /t, /step and /<plane>/vector_<k> ([n], one per
    frame), streamed through h5lite.H5Writer under a temporary name and renamed by close(), which also writes the XDMF sidecar next
    to it: a temporal collection whose frames share one Topology (Triangle, or Polyline with two nodes per element) and one XYZ
    Geometry and carry every plane as a Scalar attribute centred on the cells."""

    def __init__(self, path, spec, planes, step_offset=0, precision=8):
        from knpemidg.h5lite import H5Writer
        self.path = os.fspath(path)
        folder = os.path.dirname(os.path.abspath(self.path))
        os.makedirs(folder, exist_ok=True)
        self.tmp = os.path.join(folder, ".%s.tmp%d" % (os.path.basename(self.path), os.getpid()))
        self.spec, self.planes = spec, list(planes)
        self.t, self.step = [], []
        self.precision = int(precision)
        w = self.w = H5Writer(self.tmp)
        w.write("/surface/points", spec.points)
        w.write("/surface/connectivity", spec.connectivity.astype(np.int64))
        w.write("/surface/facet", spec.facets.astype(np.int64))
        w.write("/surface/tag", spec.tags.astype(np.int64))
        w.write("/surface/cells", spec.cells.astype(np.int64))
        w.write("/surface/area", spec.area.astype(np.float64))
        if step_offset:
            w.write("/step_offset", np.asarray([int(step_offset)], dtype=np.int64))

    def add(self, t, step, frame):
        k = len(self.t)
        for f in self.planes:
            a = np.asarray(frame[f])
            if a.shape != (self.spec.n,):
                raise ValueError("surface file: plane %r must hold one value per selected facet" % f)
            self.precision = a.dtype.itemsize
            self.w.write("/%s/vector_%d" % (f, k), a)
        self.t.append(float(t))
        self.step.append(int(step))

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
            if self.w is not None and self.w.fh is not None:
                self.w.fh.close()
            self.w = None
            if os.path.exists(self.tmp):
                os.remove(self.tmp)
        xdmf = os.path.splitext(self.path)[0] + ".xdmf"
        with open(xdmf + ".tmp%d" % os.getpid(), "w") as fh:
            fh.write(_xdmf_text(os.path.basename(self.path), self.spec, self.planes, self.t, self.precision))
        os.replace(xdmf + ".tmp%d" % os.getpid(), xdmf)
        return self.path


# ---------------------------------------------------------------------------------------------------- device
class MembraneSampler:
    """One surface sampler on the device (`Solver.record_membrane`).  sample() returns {plane: array [n]}; `facets`, `points`,
    `connectivity` describe the surface (SurfaceSpec); field_ids as resolve_fields gives them.  make_spec(membrane_tags) builds the
    SurfaceSpec once the membrane tags are known."""

    def __init__(self, make_spec, fields, field_ids, states=(), every=1, dtype=np.float64, name="membrane"):
        self.fields, self.field_ids, self.states = list(fields), list(field_ids), [str(s) for s in states]
        self.planes = check_names(self.fields, self.states)
        self.every = int(every)
        if self.every < 1:
            raise ValueError("record_membrane: every must be a positive number of steps")
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("record_membrane: dtype must be float64 or float32")
        self.name = str(name)
        if not self.name or os.sep in self.name:
            raise ValueError("record_membrane: name must be a plain file stem")
        self._make_spec, self.spec = make_spec, None
        self.dev = self.handle = None
        self._file = None
        self._waiting = []              # (t, step) of the frames enqueued on the device and not yet written
        self._scratch = None

    def resolve(self, membrane_tags):
        """Build the selection and the surface mesh (ValueError for a bad selection; no device call)."""
        if self.spec is None:
            self.spec = self._make_spec(membrane_tags)
        return self.spec

    @property
    def attached(self):
        return self.dev is not None and self.handle is not None

    def attach(self, dev, membrane_tags, models=None):
        spec = self.resolve(membrane_tags)
        tables = spec.state_tables(models or (), self.states) if self.states else None
        self.handle = dev.surf_create(spec.facets, self.field_ids, states=tables, f32=self.dtype == np.float32)
        self.dev = dev

    def _need_spec(self):
        if self.spec is None:
            raise KnpError("the membrane tags are not known yet (set up the membrane models first)")
        return self.spec

    facets = property(lambda self: self._need_spec().facets)
    points = property(lambda self: self._need_spec().points)
    connectivity = property(lambda self: self._need_spec().connectivity)

    def _need_device(self):
        if not self.attached:
            raise KnpError("the surface sampler is not on a device context yet")

    def _fetch(self, out=None):
        a = self.dev.surf_fetch(self.handle, len(self.planes), self.spec.n, self.dtype, out=out)
        return {f: a[q] for q, f in enumerate(self.planes)}

    def sample(self):
        """The planes as they are now (waits for this frame).  Not between the frames of a running time loop's file."""
        self._need_device()
        if self._waiting:
            raise KnpError("MembraneSampler.sample: frames of the time loop's file are still waiting")
        self.dev.surf_sample(self.handle)
        return self._fetch()

    def timing(self):
        """dict(sample_ms, copy_ms): kernel and copy of the last fetched frame, from HIP events."""
        self._need_device()
        return dict(zip(("sample_ms", "copy_ms"), self.dev.surf_timing(self.handle)))

    # -- the time loops' file ---------------------------------------------------------------------------------------------------
    def begin(self, filename, k0, t):
        """Open `<filename><name>[_from<k0>].h5` and enqueue frame 0: the state the loop starts from."""
        self._need_device()
        part = "_from%d" % k0 if k0 else ""
        self._file = SurfaceFile(filename + self.name + part + ".h5", self.spec, self.planes, step_offset=k0, precision=self.dtype.itemsize)
        self._enqueue(t, k0)

    def _enqueue(self, t, step):
        if self._waiting:
            self._write_one()           # frame n goes to the file while the steps queued after it run
        self.dev.surf_sample(self.handle)
        self._waiting.append((float(t), int(step)))

    def _write_one(self):
        t, step = self._waiting.pop(0)
        if self._scratch is None:       # the file takes the values at once: one buffer serves every frame of the loop
            self._scratch = np.empty((len(self.planes), self.spec.n), dtype=self.dtype)
        self._file.add(t, step, self._fetch(self._scratch))

    def after_step(self, steps_done, t):
        if self._file is not None and steps_done % self.every == 0:
            self._enqueue(t, steps_done)

    def finish(self):
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
            self.dev.surf_destroy(self.handle)
        self.dev = self.handle = None
