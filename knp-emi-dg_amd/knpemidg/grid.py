"""Fields sampled on a regular voxel grid (csrc/grid.hip): host side.

Between the recorder's handful of probes and `save_fields` (every DoF of the unstructured DG mesh) sits what people plot: a mid-plane
image of phi or [K+]_e over time, a coarse volume around an axon bundle.  The reference rebuilds such pictures from results.h5 with
FEniCS afterwards (examples/*/make_figures*.py); here `Solver.record_grid` samples them on the device while the run goes on and
writes dense arrays [nz, ny, nx] per field and frame plus an XDMF sidecar that ParaView opens.

`GridSpec` is the grid and the HOST path: a vectorised restatement of k_grid_locate / k_grid_weights / k_grid_sample, per cell over
its box of grid points, with the same arithmetic in the same order (numpy rounds every product and sum on its own; the kernels are
written to do the same).  It is what runs without a device and what the tests compare the device with.  The owner of a point
follows `recorder.locate_points`: among the cells whose smallest barycentric coordinate is >= -tol the lowest index in the caller's
numbering; a point no cell contains has owner -1 and NaN in every field.

Beside the nodal fields a grid carries what a KNP-EMI run is made for: the electric field -grad phi, the ion fluxes
J_k = -D_k grad c_k - z_k D_k psi c_k grad phi, their diffusive share and the current density F sum_k z_k J_k, evaluated in the
owner cell with that cell's D (k_grid_sample_derived; `GridSpec.sample_derived` is its host statement and also returns the sum of
the moduli of the terms of every value, the scale of a rounding bound).

`GridSampler` is what `Solver.record_grid` returns: the device handle, `sample()`, the owner and tag volumes, and the frame file
`<filename><name>.h5` (+ `<name>.xdmf`) the time loops write.
"""
import os

import numpy as np

from knpemidg._abi import GD_CURRENT, GD_EFIELD, GD_FLUX, GD_FLUX_DIFFUSIVE, KnpError
from knpemidg.recorder import basis_weights

DEFAULT_TOL = 1.0e-12
MAX_TAGS = 8               # KNP_GRID_MAX_TAGS (csrc/grid.hip)
_NONE = np.iinfo(np.int64).max


_DERIVED_PREFIXES = (("diffusive_flux_", GD_FLUX_DIFFUSIVE), ("flux_", GD_FLUX))


def resolve_fields(fields, ion_names):
    """What the C ABI samples for names out of "phi" and the ion names (ion_list order, the eliminated ion last) and out of the
    derived vector quantities "efield", "flux_<ion>", "diffusive_flux_<ion>" and "current", one entry per name in the order given:
    a nodal field is its field id (0 = phi, 1 + k = ion k), a derived quantity the pair (kind, ion) of knp_grid_create_derived
    (ion -1 for efield and current).  ValueError for an unknown or repeated name."""
    if isinstance(fields, str):
        fields = (fields,)
    ions = [str(n) for n in ion_names]
    for reserved in ("efield", "current"):
        if reserved in ions:
            raise ValueError("record_grid: an ion named %r cannot be told from the derived quantity of that name" % reserved)
    names = ["phi"] + ions
    known = names + ["efield", "current", "flux_<ion>", "diffusive_flux_<ion>"]
    out = []
    for f in fields:
        if f in names:
            entry = names.index(f)
        elif f == "efield":
            entry = (GD_EFIELD, -1)
        elif f == "current":
            entry = (GD_CURRENT, -1)
        else:
            entry = None
            for prefix, kind in _DERIVED_PREFIXES:
                if isinstance(f, str) and f.startswith(prefix) and f[len(prefix):] in ions:
                    entry = (kind, ions.index(f[len(prefix):]))
                    break
            if entry is None:
                raise ValueError("record_grid: unknown field %r (known: %s)" % (f, ", ".join(known)))
        if entry in out:
            raise ValueError("record_grid: field %r is listed twice" % (f,))
        out.append(entry)
    if not out:
        raise ValueError("record_grid: no field to sample")
    return out


def _cell_geometry(X):
    """Of the simplices X [n, d+1, d]: x0, the adjugate rows c [n, d, d] with lambda_j = ((p - x0) . c_j) / det, det, and the
    bounding box padded as recorder.locate_points pads it (grid.hip: grid_cell_geo, same operations in the same order)."""
    d = X.shape[2]
    x0 = X[:, 0, :]
    e = X[:, 1:, :] - x0[:, None, :]
    c = np.empty_like(e)
    if d == 2:
        c[:, 0, 0], c[:, 0, 1] = e[:, 1, 1], -e[:, 1, 0]
        c[:, 1, 0], c[:, 1, 1] = -e[:, 0, 1], e[:, 0, 0]
        det = e[:, 0, 0] * c[:, 0, 0] + e[:, 0, 1] * c[:, 0, 1]
    else:
        for j in range(3):
            a, b = e[:, (j + 1) % 3], e[:, (j + 2) % 3]
            c[:, j, 0] = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
            c[:, j, 1] = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
            c[:, j, 2] = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        det = (e[:, 0, 0] * c[:, 0, 0] + e[:, 0, 1] * c[:, 0, 1]) + e[:, 0, 2] * c[:, 0, 2]
    lo, hi = X.min(axis=1), X.max(axis=1)
    pad = (1.0e-9 * (hi - lo).max(axis=1))[:, None]
    return x0, c, det, lo - pad, hi + pad


def _bary(x0, c, det, p):
    """lambda [n, d+1] of the points p [n, d] in the cells given row by row (grid.hip: grid_bary)."""
    d = p.shape[1]
    r = p - x0
    lam = np.empty((len(p), d + 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(d):
            s = r[:, 0] * c[:, j, 0]
            for k in range(1, d):
                s = s + r[:, k] * c[:, j, k]
            lam[:, j + 1] = s / det
    total = lam[:, 1].copy()
    for j in range(2, d + 1):
        total = total + lam[:, j]
    lam[:, 0] = 1.0 - total
    return lam


def basis_gradients(bary, glam, degree):
    """grad w_a [n, nd, d] of the nodal basis (the local dof order of basis_weights) from lambda [n, d+1] and grad lambda
    [n, d+1, d].  P1: grad lambda_a; P2: vertices (4 lambda_a - 1) grad lambda_a, edges (a, b), a < b,
    4 (lambda_b grad lambda_a + lambda_a grad lambda_b)."""
    if degree == 1:
        return glam.copy()
    if degree != 2:
        raise ValueError("degree must be 1 or 2")
    nv = bary.shape[1]
    cols = [(4.0 * bary[:, a] - 1.0)[:, None] * glam[:, a] for a in range(nv)]
    cols += [4.0 * (bary[:, b, None] * glam[:, a] + bary[:, a, None] * glam[:, b]) for a in range(nv) for b in range(a + 1, nv)]
    return np.stack(cols, axis=1)


class GridSpec:
    """lo[d], hi[d], shape[d] (axis order x, y[, z]): point i of axis k is lo[k] + i h[k], h[k] = (hi[k] - lo[k]) / (shape[k] - 1);
    an axis with shape[k] == 1 sits at lo[k] -- a slice of a 3D mesh.  tags: restrict the candidate cells to these subdomains (the
    side of a point on a membrane; ECS-only or ICS-only images).  Arrays of point values are shaped shape[::-1]: [nz, ny, nx]."""

    def __init__(self, dim, lo, hi, shape, tol=DEFAULT_TOL, tags=None):
        self.dim = int(dim)
        try:
            lo, hi = np.array(lo, dtype=np.float64).ravel(), np.array(hi, dtype=np.float64).ravel()
            shp = np.array(shape).ravel()
        except (TypeError, ValueError):
            raise ValueError("grid: lo, hi and shape must be sequences of numbers")
        if lo.shape != (self.dim,) or hi.shape != (self.dim,) or shp.shape != (self.dim,):
            raise ValueError("grid: lo, hi and shape must hold one entry per mesh dimension (%d)" % self.dim)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError("grid: the bounds must be finite")
        if shp.dtype.kind not in "iu" and not (np.isfinite(shp.astype(np.float64)).all() and (shp == np.round(shp)).all()):
            raise ValueError("grid: shape must hold whole numbers")
        shp = shp.astype(np.int64)
        if (shp < 1).any():
            raise ValueError("grid: every entry of shape must be at least 1")
        if np.prod(shp.astype(np.float64)) >= 2.0 ** 31:
            raise ValueError("grid: the grid must hold fewer than 2^31 points")
        if ((shp > 1) & ~(hi > lo)).any():
            raise ValueError("grid: hi must lie above lo along every axis with more than one point")
        if not (np.isfinite(tol) and tol >= 0.0):
            raise ValueError("grid: tol must be finite and not negative")
        self.lo, self.hi, self.shape, self.tol = lo, hi, shp, float(tol)
        self.h = np.where(shp > 1, (hi - lo) / np.maximum(shp - 1, 1), 0.0)
        self.tags = None if tags is None else tuple(int(t) for t in np.atleast_1d(tags))
        if self.tags is not None and not 1 <= len(self.tags) <= MAX_TAGS:
            raise ValueError("grid: between 1 and %d subdomain tags" % MAX_TAGS)
        self.npts = int(np.prod(shp))
        self.owner = self.bary = None

    @property
    def array_shape(self):
        return tuple(int(n) for n in self.shape[::-1])

    def axis(self, k):
        return self.lo[k] + np.arange(self.shape[k], dtype=np.int64).astype(np.float64) * self.h[k]

    def points(self):
        """[npts, d] coordinates, x fastest."""
        ax = [self.axis(k) for k in range(self.dim)]
        mesh = np.meshgrid(*ax[::-1], indexing="ij")
        return np.stack([m.ravel() for m in mesh[::-1]], axis=1)

    def _ranges(self, k, blo, bhi):
        """[i0, i1] and validity of the indices of axis k that can lie in [blo, bhi] (grid.hip: grid_range)."""
        n = int(self.shape[k])
        if n == 1:
            z = np.zeros(len(blo), dtype=np.int64)
            return z, z.copy(), np.ones(len(blo), dtype=bool)
        a = np.floor((blo - self.lo[k]) / self.h[k]) - 1.0
        b = np.ceil((bhi - self.lo[k]) / self.h[k]) + 1.0
        ok = (a <= n - 1) & (b >= 0.0)
        i0 = np.clip(np.where(ok, a, 0.0), 0, n - 1).astype(np.int64)
        i1 = np.clip(np.where(ok, b, 0.0), 0, n - 1).astype(np.int64)
        return i0, i1, ok & (i0 <= i1)

    def locate(self, mesh, cell_tags=None, chunk=1 << 21):
        """owner [npts] (int64, -1 outside) and bary [npts, d+1] (0 outside); also kept as self.owner / self.bary."""
        d = self.dim
        if mesh.gdim != d:
            raise ValueError("grid: the mesh has dimension %d, the grid %d" % (mesh.gdim, d))
        cells = np.asarray(mesh.cells)
        coords = np.asarray(mesh.coords, dtype=np.float64)
        cand = np.arange(len(cells), dtype=np.int64)
        if self.tags is not None:
            if cell_tags is None:
                raise ValueError("grid: tags need the cell tags")
            cand = cand[np.isin(np.asarray(cell_tags), self.tags)]
        owner = np.full(self.npts, _NONE, dtype=np.int64)
        x0, c, det, blo, bhi = _cell_geometry(coords[cells[cand]])
        i0, cnt, ok = [], [], np.ones(len(cand), dtype=bool)
        for k in range(d):
            a, b, v = self._ranges(k, blo[:, k], bhi[:, k])
            i0.append(a)
            cnt.append(b - a + 1)
            ok &= v
        total = np.where(ok, np.prod(np.stack(cnt), axis=0), 0)
        nx, ny = int(self.shape[0]), int(self.shape[1])
        edges = np.concatenate([[0], np.cumsum(total)])
        first = 0
        while first < len(cand):
            last = max(int(np.searchsorted(edges, edges[first] + chunk, side="right")) - 1, first + 1)
            sel = np.arange(first, last)
            first = last
            tot = total[sel]
            if not tot.sum():
                continue
            which = np.repeat(sel, tot)                                   # position in `cand` of every (cell, point) pair
            local = np.arange(int(tot.sum()), dtype=np.int64) - np.repeat(np.cumsum(tot) - tot, tot)
            idx = []
            for k in range(d):
                ck = cnt[k][which]
                idx.append(i0[k][which] + local % ck)
                local = local // ck
            p = np.stack([self.lo[k] + idx[k].astype(np.float64) * self.h[k] for k in range(d)], axis=1)
            inside = np.all((p >= blo[which]) & (p <= bhi[which]), axis=1)
            which, p, idx = which[inside], p[inside], [i[inside] for i in idx]
            lam = _bary(x0[which], c[which], det[which], p)
            hit = lam.min(axis=1) >= -self.tol
            flat = idx[1] * nx + idx[0] if d == 2 else (idx[2] * ny + idx[1]) * nx + idx[0]
            np.minimum.at(owner, flat[hit], cand[which[hit]])
        owner[owner == _NONE] = -1
        bary = np.zeros((self.npts, d + 1))
        found = np.nonzero(owner >= 0)[0]
        if len(found):
            g = _cell_geometry(coords[cells[owner[found]]])
            bary[found] = _bary(g[0], g[1], g[2], self.points()[found])
        self.owner, self.bary = owner, bary
        return owner, bary

    def sample(self, u, degree, owner=None, bary=None):
        """Values [npts] of the nodal field u [nc, nd] (caller's cell order): sum_a w_a(lambda) u[cell, a], NaN where owner is -1."""
        owner = self.owner if owner is None else owner
        bary = self.bary if bary is None else bary
        if owner is None:
            raise ValueError("grid: locate the points first")
        u = np.asarray(u, dtype=np.float64)
        w = basis_weights(bary, degree)
        u = u.reshape(-1, w.shape[1])
        out = np.full(self.npts, np.nan)
        found = owner >= 0
        out[found] = (w[found] * u[owner[found]]).sum(axis=1)
        return out

    def sample_derived(self, mesh, quantities, phi, conc, z, D, psi, F, degree, owner=None, bary=None):
        """The host statement of k_grid_sample_derived.  quantities: (kind, ion) pairs as resolve_fields gives them; phi [nc, nd] and
        conc [n_ions][nc, nd] the nodal fields (caller's cell order, the eliminated ion last); z [n_ions], D [n_ions][nc], psi = F / (R T).
        With grad u = sum_a u_a grad w_a and u(p) = sum_a u_a w_a in the owner cell, grad lambda_j = c_j / det from _cell_geometry:
          efield -grad phi;  diffusive flux -D_k grad c_k;  flux J_k = -D_k grad c_k - z_k D_k psi c_k(p) grad phi;
          current F sum_k z_k J_k over every ion.
        Returns (values, scale), each [len(quantities), npts, d]: values are NaN where owner is -1; scale is, per point and component,
        the sum of the absolute values of the terms the value is made of (every u_a grad w_a and u_a w_a entering with its
        modulus; 0 where owner is -1) -- what a rounding bound for the value has to be proportional to."""
        owner = self.owner if owner is None else owner
        bary = self.bary if bary is None else bary
        if owner is None:
            raise ValueError("grid: locate the points first")
        d = self.dim
        z, D = np.asarray(z, dtype=np.float64), np.asarray(D, dtype=np.float64)
        n_ions = len(z)
        found = np.nonzero(owner >= 0)[0]
        cells = owner[found]
        _, c, det, _, _ = _cell_geometry(np.asarray(mesh.coords, dtype=np.float64)[np.asarray(mesh.cells)[cells]])
        glam = np.empty((len(found), d + 1, d))
        glam[:, 1:] = c / det[:, None, None]
        glam[:, 0] = -glam[:, 1:].sum(axis=1)
        w = basis_weights(bary[found], degree)
        dw = basis_gradients(bary[found], glam, degree)
        aw, adw = np.abs(w), np.abs(dw)

        def value_grad(u):
            u = np.asarray(u, dtype=np.float64).reshape(-1, w.shape[1])[cells]
            return ((w * u).sum(axis=1), np.einsum("na,nak->nk", u, dw),
                    (aw * np.abs(u)).sum(axis=1), np.einsum("na,nak->nk", np.abs(u), adw))

        _, gphi, _, aphi = value_grad(phi)
        ion_cache = {}

        def ion_terms(k):
            """(diffusive flux, flux, their scales) of ion k"""
            if k not in ion_cache:
                ck, gck, ack, agck = value_grad(conc[k])
                Dk = D[k][cells][:, None]
                diff, sdiff = -Dk * gck, Dk * agck
                drift = z[k] * Dk * psi * ck[:, None]
                ion_cache[k] = (diff, diff - drift * gphi, sdiff, sdiff + np.abs(z[k]) * Dk * psi * ack[:, None] * aphi)
            return ion_cache[k]

        values = np.full((len(quantities), self.npts, d), np.nan)
        scale = np.zeros((len(quantities), self.npts, d))
        for q, (kind, ion) in enumerate(quantities):
            if kind == GD_EFIELD:
                v, s = -gphi, aphi
            elif kind == GD_FLUX_DIFFUSIVE:
                v, _, s, _ = ion_terms(ion)
            elif kind == GD_FLUX:
                _, v, _, s = ion_terms(ion)
            elif kind == GD_CURRENT:
                v, s = np.zeros_like(gphi), np.zeros_like(gphi)
                for k in range(n_ions):
                    _, fk, _, sk = ion_terms(k)
                    v = v + F * z[k] * fk
                    s = s + F * np.abs(z[k]) * sk
            else:
                raise ValueError("grid: unknown derived quantity %r" % (kind,))
            values[q, found], scale[q, found] = v, s
        return values, scale


# ---------------------------------------------------------------------------------------------------- files
def _xdmf_text(h5_name, spec, fields, times, precision, vectors=()):
    d = spec.dim
    dims = " ".join(str(n) for n in spec.array_shape)
    topo, geo = ("3DCoRectMesh", "ORIGIN_DXDYDZ") if d == 3 else ("2DCoRectMesh", "ORIGIN_DXDY")
    vec = lambda v: " ".join(repr(float(x)) for x in v[::-1])
    # a CoRectMesh needs a positive spacing on every axis, also on one that holds a single point
    spacing = np.where(spec.shape > 1, spec.h, 1.0)
    out = ['<?xml version="1.0" ?>', '<Xdmf Version="3.0">', ' <Domain>',
           '  <Grid Name="%s" GridType="Collection" CollectionType="Temporal">' % os.path.splitext(h5_name)[0]]
    for n, t in enumerate(times):
        out += ['   <Grid Name="frame_%d" GridType="Uniform">' % n,
                '    <Time Value="%r"/>' % float(t),
                '    <Topology TopologyType="%s" Dimensions="%s"/>' % (topo, dims),
                '    <Geometry GeometryType="%s">' % geo,
                '     <DataItem Format="XML" Dimensions="%d">%s</DataItem>' % (d, vec(spec.lo)),
                '     <DataItem Format="XML" Dimensions="%d">%s</DataItem>' % (d, vec(spacing)),
                '    </Geometry>']
        for f in fields:
            # a Vector attribute has three components, also on a 2D grid (GridFile.add writes a zero third one)
            kind, fdims = ("Vector", dims + " 3") if f in vectors else ("Scalar", dims)
            out += ['    <Attribute Name="%s" AttributeType="%s" Center="Node">' % (f, kind),
                    '     <DataItem Format="HDF" NumberType="Float" Precision="%d" Dimensions="%s">%s:/%s/vector_%d</DataItem>'
                    % (precision, fdims, h5_name, f, n),
                    '    </Attribute>']
        out.append('   </Grid>')
    out += ['  </Grid>', ' </Domain>', '</Xdmf>', '']
    return "\n".join(out)


class GridFile:
    """`path` (.h5) with /grid/{lo,hi,shape,spacing}, /grid/cell, /grid/tag, /t, /step and /<field>/vector_<n> ([nz, ny, nx]; a vector
    quantity, handed to add() as [..., d], is written as [nz, ny, nx, 3] and declared AttributeType="Vector"), streamed through
    h5lite.H5Writer under a temporary name and renamed by close(), which also writes the XDMF sidecar next to it: a
    3DCoRectMesh / 2DCoRectMesh temporal collection (Dimensions, Origin and DxDyDz in z-y-x order) whose DataItems point into the .h5."""

    def __init__(self, path, spec, fields, cell, tag, step_offset=0):
        from knpemidg.h5lite import H5Writer
        self.path = os.fspath(path)
        folder = os.path.dirname(os.path.abspath(self.path))
        os.makedirs(folder, exist_ok=True)
        self.tmp = os.path.join(folder, ".%s.tmp%d" % (os.path.basename(self.path), os.getpid()))
        self.spec, self.fields = spec, list(fields)
        self.t, self.step = [], []
        self.vectors = set()            # the fields whose frames came as [..., d]: Vector attributes of the sidecar
        self.precision = 8
        w = self.w = H5Writer(self.tmp)
        w.write("/grid/lo", spec.lo)
        w.write("/grid/hi", spec.hi)
        w.write("/grid/shape", spec.shape.astype(np.int64))
        w.write("/grid/spacing", spec.h)
        w.write("/grid/cell", np.asarray(cell, dtype=np.int64).reshape(spec.array_shape))
        w.write("/grid/tag", np.asarray(tag, dtype=np.int64).reshape(spec.array_shape))
        if step_offset:
            w.write("/step_offset", np.asarray([int(step_offset)], dtype=np.int64))

    def add(self, t, step, frame):
        n = len(self.t)
        shape = self.spec.array_shape
        for f in self.fields:
            a = np.asarray(frame[f])
            self.precision = a.dtype.itemsize
            if a.ndim == len(shape) + 1:
                # a vector quantity [..., d] (a view into the component planes of the frame): interleaved here, in the one copy the
                # writer makes anyway, as [..., 3] with a zero third component in 2D
                self.vectors.add(f)
                v = np.zeros(shape + (3,), dtype=a.dtype)
                v[..., :a.shape[-1]] = a
                a = v
            self.w.write("/%s/vector_%d" % (f, n), a.reshape(shape + a.shape[len(shape):]))
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
            fh.write(_xdmf_text(os.path.basename(self.path), self.spec, self.fields, self.t, self.precision, self.vectors))
        os.replace(xdmf + ".tmp%d" % os.getpid(), xdmf)
        return self.path


# ---------------------------------------------------------------------------------------------------- device
class GridSampler:
    """One grid on the device (`Solver.record_grid`).  sample() returns {field: array shaped shape[::-1]}, a vector quantity (efield,
    flux_<ion>, diffusive_flux_<ion>, current) shaped shape[::-1] + (d,); field_ids as resolve_fields gives them; `cells` and `tags` are
    the owner (caller's cell ids) and subdomain volumes, -1 where the grid sticks out of the mesh."""

    def __init__(self, spec, fields, field_ids, every=1, dtype=np.float64, name="grid"):
        self.spec, self.fields, self.field_ids = spec, list(fields), list(field_ids)
        # the layout of a frame: the nodal planes in the order given, then d component planes per derived quantity in the order given
        self.nodal = [(f, e) for f, e in zip(self.fields, self.field_ids) if not isinstance(e, tuple)]
        self.derived = [(f, e) for f, e in zip(self.fields, self.field_ids) if isinstance(e, tuple)]
        self.n_planes = len(self.nodal) + spec.dim * len(self.derived)
        self.every = int(every)
        if self.every < 1:
            raise ValueError("record_grid: every must be a positive number of steps")
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("record_grid: dtype must be float64 or float32")
        self.name = str(name)
        if not self.name or os.sep in self.name:
            raise ValueError("record_grid: name must be a plain file stem")
        self.dev = self.handle = None
        self._points = None
        self._file = None
        self._waiting = []              # (t, step) of the frames enqueued on the device and not yet written
        self._scratch = None

    def attach(self, dev):
        s = self.spec
        self.handle = dev.grid_create(s.lo, s.h, s.shape, [e for _, e in self.nodal], tol=s.tol, tags=s.tags, f32=self.dtype == np.float32,
                                      derived=[e for _, e in self.derived] or None)
        self.dev = dev
        self._points = None

    def _need_device(self):
        if self.dev is None or self.handle is None:
            raise KnpError("the grid is not on a device context yet")

    def _volumes(self):
        self._need_device()
        if self._points is None:
            owner, tag = self.dev.grid_points(self.handle, self.spec.npts)
            self._points = (owner.reshape(self.spec.array_shape), tag.reshape(self.spec.array_shape))
        return self._points

    @property
    def cells(self):
        return self._volumes()[0]

    @property
    def tags(self):
        return self._volumes()[1]

    def _fetch(self, out=None):
        a = self.dev.grid_fetch(self.handle, self.n_planes, self.spec.npts, self.dtype, out=out)
        shape, d, nn = self.spec.array_shape, self.spec.dim, len(self.nodal)
        frame = {f: a[q].reshape(shape) for q, (f, _) in enumerate(self.nodal)}
        for q, (f, _) in enumerate(self.derived):
            # [..., d], x component first: a view of the quantity's component planes
            frame[f] = np.moveaxis(a[nn + q * d:nn + (q + 1) * d].reshape((d,) + shape), 0, -1)
        return frame

    def sample(self):
        """The fields as they are now (waits for this frame).  Not between the frames of a running time loop's file."""
        self._need_device()
        if self._waiting:
            raise KnpError("GridSampler.sample: frames of the time loop's file are still waiting")
        self.dev.grid_sample(self.handle)
        return self._fetch()

    def timing(self):
        """dict(locate_ms, weights_ms, sample_ms, copy_ms): the two one-time passes and the last fetched frame, from HIP events."""
        self._need_device()
        return dict(zip(("locate_ms", "weights_ms", "sample_ms", "copy_ms"), self.dev.grid_timing(self.handle)))

    # -- the time loops' file ---------------------------------------------------------------------------------------------------
    def begin(self, filename, k0, t):
        """Open `<filename><name>[_from<k0>].h5` and enqueue frame 0: the state the loop starts from."""
        self._need_device()
        part = "_from%d" % k0 if k0 else ""
        self._file = GridFile(filename + self.name + part + ".h5", self.spec, self.fields, self.cells, self.tags, step_offset=k0)
        self._enqueue(t, k0)

    def _enqueue(self, t, step):
        if self._waiting:
            self._write_one()           # frame n goes to the file while the steps queued after it run
        self.dev.grid_sample(self.handle)
        self._waiting.append((float(t), int(step)))

    def _write_one(self):
        t, step = self._waiting.pop(0)
        if self._scratch is None:       # the file takes the values at once: one buffer serves every frame of the loop
            self._scratch = np.empty((self.n_planes, self.spec.npts), dtype=self.dtype)
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
        if self.dev is not None and self.handle is not None and getattr(self.dev, "ctx", None):
            self.dev.grid_destroy(self.handle)
        self.dev = self.handle = None
