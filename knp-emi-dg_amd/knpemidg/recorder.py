"""Time series sampled on the device: point probes, membrane-set means and region integrals (csrc/record.hip).

The reference has no such path: its figure scripts (examples/idealized-geometries/make_figures_3D.py:28-168) evaluate phi and the
concentrations at a few points, average phi_M / E_K / E_Na over the membrane facets inside a small box and integrate over
subdomains, all from the full fields that `save_fields=True, sf=1` wrote at every step.  Here `Solver.record(...)` attaches a
`Recorder`; after step III of every time step one row is appended to a small device buffer, which comes back in one copy per
`capacity` steps.  The host part below only prepares tables: containing cell and basis values of every probe, facet lists with
area weights, a region id and the volume of every cell.
"""
import numpy as np

from knpemidg._abi import KnpError

REGION_NONE = 255          # region id of a cell that no region integral counts
MAX_REGIONS = 16           # KNP_REC_MAX_REGIONS (csrc/record.hip)


# ---------------------------------------------------------------------------- geometry helpers (host)
def cell_volumes(mesh):
    X = mesh.coords[mesh.cells]
    d = mesh.gdim
    J = X[:, 1:, :] - X[:, :1, :]
    return np.abs(np.linalg.det(J)) / (2.0 if d == 2 else 6.0)


def facet_areas(mesh, facets):
    """Length (2D) / area (3D) of the given facets."""
    X = mesh.coords[mesh.facets[np.asarray(facets, dtype=np.int64)]]
    if mesh.gdim == 2:
        return np.linalg.norm(X[:, 1] - X[:, 0], axis=1)
    return 0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)


def barycentric(X, p):
    """Barycentric coordinates [n, d+1] of point p in the simplices X [n, d+1, d]."""
    X = np.asarray(X, dtype=np.float64)
    T = (X[:, 1:, :] - X[:, :1, :]).transpose(0, 2, 1)
    rhs = (np.asarray(p, dtype=np.float64)[None, :] - X[:, 0, :])[:, :, None]
    lam = np.linalg.solve(T, rhs)[:, :, 0]
    return np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1)


def basis_weights(bary, degree):
    """Values of the nodal basis at barycentric points [n, d+1] -> [n, nd].  P1: the coordinates themselves; P2: the quadratic
    Lagrange basis in this project's local dof order (vertices, then the edge midpoints (a, b), a < b, lexicographic)."""
    lam = np.atleast_2d(np.asarray(bary, dtype=np.float64))
    if degree == 1:
        return lam.copy()
    if degree != 2:
        raise ValueError("degree must be 1 or 2")
    nv = lam.shape[1]
    cols = [lam[:, a] * (2.0 * lam[:, a] - 1.0) for a in range(nv)]
    cols += [4.0 * lam[:, a] * lam[:, b] for a in range(nv) for b in range(a + 1, nv)]
    return np.stack(cols, axis=1)


def nodal_integration_weights(dim, degree):
    """w [nd] with  int_K u dx = vol_K sum_a w[a] u_a  exactly for nodal data of degree `degree` (the weights of k_rec_regions)."""
    nv = dim + 1
    if degree == 1:
        return np.full(nv, 1.0 / nv)
    if degree != 2:
        raise ValueError("degree must be 1 or 2")
    ne = nv * (nv - 1) // 2
    if dim == 2:
        return np.concatenate([np.zeros(nv), np.full(ne, 1.0 / 3.0)])
    return np.concatenate([np.full(nv, -1.0 / 20.0), np.full(ne, 1.0 / 5.0)])


def locate_points(mesh, points, cell_tags=None, point_tags=None, tol=1.0e-12):
    """Containing cell (caller's numbering) and barycentric coordinates of every point.  Of several cells that contain a point --
    it sits on a facet, an edge or a vertex -- the one with the lowest index wins; `tol` is the barycentric tolerance, i.e. 1e-12 of
    the cell size.  point_tags[i] (None = any) restricts point i to the cells of that subdomain, which decides the side of a point
    on a membrane.  A point that no cell contains raises ValueError."""
    pts = np.atleast_2d(np.asarray(points, dtype=np.float64))
    d = mesh.gdim
    if pts.shape[1] != d:
        raise ValueError("points must have shape [n, %d]" % d)
    lo = mesh.coords[mesh.cells[:, 0]].copy()
    hi = lo.copy()
    for a in range(1, d + 1):
        xa = mesh.coords[mesh.cells[:, a]]
        np.minimum(lo, xa, out=lo)
        np.maximum(hi, xa, out=hi)
    pad = 1.0e-9 * (hi - lo).max(axis=1)[:, None]            # bounding-box prefilter only; the barycentric test decides
    lo -= pad
    hi += pad
    tags = None if cell_tags is None else np.asarray(cell_tags)
    cells = np.empty(len(pts), dtype=np.int64)
    bary = np.empty((len(pts), d + 1))
    for i, p in enumerate(pts):
        cand = np.nonzero(np.all((p >= lo) & (p <= hi), axis=1))[0]
        want = None if point_tags is None else point_tags[i]
        if want is not None:
            if tags is None:
                raise ValueError("point_tags need the cell tags")
            cand = cand[tags[cand] == int(want)]
        lam = barycentric(mesh.coords[mesh.cells[cand]], p) if len(cand) else np.zeros((0, d + 1))
        ok = np.nonzero(lam.min(axis=1) >= -tol)[0]
        if not len(ok):
            raise ValueError("probe point %d %s lies outside the mesh%s" % (i, tuple(float(x) for x in p),
                                                                              "" if want is None else " (subdomain %d)" % int(want)))
        cells[i] = cand[ok[0]]                                # cand is ascending: the lowest cell index
        bary[i] = lam[ok[0]]
    return cells, bary


def membrane_facets(mesh, facet_tags, membrane_tags):
    """Ids of the membrane facets: interior facets whose tag is one of membrane_tags (what knp_ctx_create classifies as membrane)."""
    ft = np.asarray(facet_tags)
    return np.nonzero((mesh.facet_cells[:, 1] >= 0) & np.isin(ft, list(membrane_tags)))[0]


def select_box(mesh, facets, lo, hi):
    """The facets of `facets` whose midpoint lies in the closed box [lo, hi] (make_figures_3D.py:95-107)."""
    facets = np.asarray(facets, dtype=np.int64)
    mid = mesh.facet_midpoints()[facets]
    inside = np.all((mid >= np.asarray(lo, dtype=np.float64)) & (mid <= np.asarray(hi, dtype=np.float64)), axis=1)
    return facets[inside]


def _is_box(entry, d):
    try:
        a = np.asarray(entry, dtype=np.float64)
    except (ValueError, TypeError):
        return False
    return a.shape == (2, d)


class Recorder:
    """Tables of one recorder and the samples read back so far.

    points        [n, dim] probe coordinates (point_tags: optional subdomain per probe)
    membrane_sets list of facet-id arrays or (lo, hi) boxes
    regions       True: one region per distinct subdomain tag, ascending; False / None: none; or an array [nc] of region ids
                  (255 = not counted)
    ion_names     names in ion_list order (the eliminated ion last)
    """

    def __init__(self, mesh, cell_tags, facet_tags, degree, ion_names, points=None, membrane_sets=None, regions=True, capacity=256,
                 point_tags=None, membrane_tags=None):
        self.mesh = mesh
        self.cell_tags = np.asarray(cell_tags)
        self.facet_tags = np.asarray(facet_tags)
        self.degree = int(degree)
        self.ion_names = list(ion_names)
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be positive")
        d = mesh.gdim
        self.nd = d + 1 if self.degree == 1 else (d + 1) * (d + 2) // 2
        # probes
        self.point_coords = np.zeros((0, d)) if points is None else np.atleast_2d(np.asarray(points, dtype=np.float64)).copy()
        if point_tags is not None and len(point_tags) != len(self.point_coords):
            raise ValueError("point_tags must hold one entry per point")
        self.point_cells, self.point_bary = locate_points(mesh, self.point_coords, self.cell_tags, point_tags) \
            if len(self.point_coords) else (np.zeros(0, dtype=np.int64), np.zeros((0, d + 1)))
        self.point_w = basis_weights(self.point_bary, self.degree) if len(self.point_coords) else np.zeros((0, self.nd))
        # regions
        nc = mesh.num_cells()
        if regions is True:
            self.region_tags = [int(t) for t in np.unique(self.cell_tags)]
            self.region = np.searchsorted(np.asarray(self.region_tags), self.cell_tags).astype(np.uint8) \
                if len(self.region_tags) <= MAX_REGIONS else None
        elif regions is None or regions is False:
            self.region_tags, self.region = [], np.full(nc, REGION_NONE, dtype=np.uint8)
        else:
            self.region = np.ascontiguousarray(regions, dtype=np.uint8)
            if self.region.shape != (nc,):
                raise ValueError("regions must hold one id per cell")
            used = self.region[self.region != REGION_NONE]
            self.region_tags = list(range(int(used.max()) + 1)) if len(used) else []
        if self.region is None or len(self.region_tags) > MAX_REGIONS:
            raise ValueError("at most %d regions" % MAX_REGIONS)
        self.vol = cell_volumes(mesh)
        # membrane sets: resolved once the membrane tags are known
        self._set_spec = list(membrane_sets) if membrane_sets is not None else []
        self.set_facets = None
        if membrane_tags is not None:
            self.resolve_sets(membrane_tags)
        self.dev = None
        self._t = []
        self._rows = []
        self._waiting = 0               # rows in the device buffer

    # -- tables -----------------------------------------------------------------
    def resolve_sets(self, membrane_tags):
        mesh = self.mesh
        mem = membrane_facets(mesh, self.facet_tags, membrane_tags)
        out = []
        for i, entry in enumerate(self._set_spec):
            if _is_box(entry, mesh.gdim):
                f = select_box(mesh, mem, entry[0], entry[1])
            else:
                f = np.asarray(entry, dtype=np.int64).ravel()
                bad = f[~np.isin(f, mem)]
                if len(bad):
                    raise ValueError("membrane set %d: facet %d is not a membrane facet" % (i, int(bad[0])))
            if not len(f):
                raise ValueError("membrane set %d is empty" % i)
            out.append(f)
        self.set_facets = out
        self.set_weights = []
        for f in out:
            a = facet_areas(mesh, f)
            self.set_weights.append(a / a.sum())

    @property
    def n_points(self):
        return len(self.point_coords)

    @property
    def n_sets(self):
        return len(self._set_spec)

    @property
    def n_regions(self):
        return len(self.region_tags)

    def channel_names(self):
        """(point names, membrane names, region names) in row order."""
        ions = self.ion_names
        return (["phi"] + ions, ["phi_M"] + ["E_" + n for n in ions] + ["I_ch_" + n for n in ions], ions + ["phi_mean"])

    def attach(self, dev, membrane_tags=None):
        """Create the device recorder on `dev` (a knpemidg._abi.Device without ghost cells)."""
        if self.set_facets is None:
            self.resolve_sets(membrane_tags if membrane_tags is not None else [])
        ptr = np.concatenate([[0], np.cumsum([len(f) for f in self.set_facets])]).astype(np.int64)
        sf = np.concatenate(self.set_facets) if self.set_facets else np.zeros(0, dtype=np.int64)
        sw = np.concatenate(self.set_weights) if self.set_facets else np.zeros(0)
        self.n_channels = dev.rec_create(self.capacity, self.point_cells, self.point_w, ptr, sf, sw, self.n_regions, self.region, self.vol)
        n_ions = len(self.ion_names)
        assert self.n_channels == self.n_points * (n_ions + 1) + self.n_sets * (1 + 2 * n_ions) + self.n_regions * (n_ions + 1)
        self.dev = dev
        self._waiting = 0

    # -- sampling -----------------------------------------------------------------
    def sample(self, t):
        """One row at time t (asynchronous).  A full device buffer is read back first: the only synchronisation."""
        if self.dev is None:
            raise KnpError("the recorder is not attached to a device context yet")
        if self._waiting >= self.capacity:
            self.flush()
        self.dev.rec_sample(float(t))
        self._waiting += 1

    def flush(self):
        if self.dev is None or not self._waiting:
            return
        t, rows = self.dev.rec_read()
        assert len(t) == self._waiting
        self._t.append(t)
        self._rows.append(rows)
        self._waiting = 0

    # -- results ------------------------------------------------------------------
    @property
    def rows(self):
        """All samples so far, [n_steps, n_channels] in the row layout of include/knpemi_hip.h."""
        self.flush()
        if not self._rows:
            return np.zeros((0, getattr(self, "n_channels", 0)))
        if len(self._rows) > 1:
            self._rows, self._t = [np.concatenate(self._rows)], [np.concatenate(self._t)]
        return self._rows[0]

    @property
    def t(self):
        r = self.rows
        return self._t[0] if len(r) else np.zeros(0)

    def _block(self, first, n_items, names):
        r = self.rows
        nq = len(names)
        blk = r[:, first:first + n_items * nq].reshape(len(r), n_items, nq)
        return {name: np.ascontiguousarray(blk[:, :, q]) for q, name in enumerate(names)}

    @property
    def points(self):
        return self._block(0, self.n_points, self.channel_names()[0])

    @property
    def membrane(self):
        n_ions = len(self.ion_names)
        return self._block(self.n_points * (n_ions + 1), self.n_sets, self.channel_names()[1])

    @property
    def regions(self):
        n_ions = len(self.ion_names)
        return self._block(self.n_points * (n_ions + 1) + self.n_sets * (1 + 2 * n_ions), self.n_regions, self.channel_names()[2])

    def save(self, path):
        """/timeseries/t, /timeseries/points/<name>, /timeseries/membrane/<name>, /timeseries/regions/<name> ([n_steps, n_items]) plus
        the probe coordinates and cells, the facets and weights of every membrane set and the region tags."""
        import os
        from knpemidg.h5lite import H5Writer
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with H5Writer(path) as w:
            w.write("/timeseries/t", self.t)
            for group, data, n in (("points", self.points, self.n_points), ("membrane", self.membrane, self.n_sets),
                                   ("regions", self.regions, self.n_regions)):
                if n:
                    for name, a in data.items():
                        w.write("/timeseries/%s/%s" % (group, name), a)
            if self.n_points:
                w.write("/probes/coordinates", self.point_coords)
                w.write("/probes/cells", self.point_cells.astype(np.int64))
            for i in range(self.n_sets):
                w.write("/membrane_sets/set_%d/facets" % i, self.set_facets[i].astype(np.int64))
                w.write("/membrane_sets/set_%d/weights" % i, self.set_weights[i])
            if self.n_regions:
                w.write("/regions/tags", np.asarray(self.region_tags, dtype=np.int64))
        return path
