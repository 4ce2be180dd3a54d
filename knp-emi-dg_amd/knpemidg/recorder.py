"""Time series sampled on the device: point probes, membrane-set means and region integrals (csrc/record.hip).

The reference has no such path: its figure scripts (examples/idealized-geometries/make_figures_3D.py:28-168) evaluate phi and the
concentrations at a few points, average phi_M / E_K / E_Na over the membrane facets inside a small box and integrate over
subdomains, all from the full fields that `save_fields=True, sf=1` wrote at every step.  Here `Solver.record(...)` attaches a
`Recorder`; after step III of every time step one row is appended to a small device buffer, which comes back in one copy per
`capacity` steps.  The host part below only prepares tables: containing cell and basis values of every probe, facet lists with
area weights, a region id and the volume of every cell.

Two optional additions serve the reference's other figure scripts (examples/rat-neuron/make_figures_rat_neuron.py:238-315, 423-692):
`membrane_states` appends the area-weighted means of ODE state columns (the gating variables n, m, h) over the membrane sets, read
straight from the state tables on the device, and `membrane_map` keeps a per-facet activation map (activation and repolarisation
time, peak, number of activations) from which `Recorder.conduction_velocity` follows.

Partitioned runs (knpemidg/partition.py): the recorder is built from the GLOBAL mesh on every rank and `localize_tables` cuts out what
the rank owns -- a probe belongs to the rank that owns its cell, a membrane facet to the rank that owns its first cell, a cell's
volume to its owner -- with the global weights, so that the ranks' partial rows add up to the one-GPU row.  Nothing is communicated
per sample; the partial rows are summed over the ranks when the device buffer is read, which makes every read a collective call.
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


def model_has_state(ode, name):
    try:
        ode.state_indices(name)
    except (ValueError, KeyError):
        return False
    return True


def state_entries(set_facets, set_areas, models, names):
    """Entry lists of the state channels, channel = set * len(names) + name (knp_rec_add_states).

    models: the membrane models -- anything with `facets` (ascending facet ids; row r of the state table belongs to facets[r]),
    `ode.state_indices(name)` (ValueError for a name the model does not have) and `handle` (the device ODE handle).
    Channel (s, q) is the mean of state q over those facets of set s whose model has a state q, in the set's facet order, weighted
    by the facet areas renormalised over exactly those facets.  Returns (chan_ptr, handle, row, col, weight); ValueError naming
    the set and the state when no facet of the set has it."""
    owner, row_of = {}, {}
    for k, m in enumerate(models):
        for r, f in enumerate(np.asarray(m.facets, dtype=np.int64)):
            owner[int(f)] = k
            row_of[int(f)] = r
    cols = [{q: (m.ode.state_indices(q) if model_has_state(m.ode, q) else None) for q in names} for m in models]
    ptr, eh, er, ec, ew = [0], [], [], [], []
    for s, (facets, areas) in enumerate(zip(set_facets, set_areas)):
        facets = np.asarray(facets, dtype=np.int64)
        areas = np.asarray(areas, dtype=np.float64)
        for q in names:
            keep = [i for i, f in enumerate(facets) if int(f) in owner and cols[owner[int(f)]][q] is not None]
            if not keep:
                raise ValueError("membrane set %d: no facet of the set belongs to a membrane model with a state '%s'" % (s, q))
            w = areas[keep] / areas[keep].sum()
            for i, wi in zip(keep, w):
                k = owner[int(facets[i])]
                eh.append(int(models[k].handle))
                er.append(row_of[int(facets[i])])
                ec.append(int(cols[k][q]))
                ew.append(float(wi))
            ptr.append(len(eh))
    return (np.asarray(ptr, dtype=np.int64), np.asarray(eh, dtype=np.int32), np.asarray(er, dtype=np.int64),
            np.asarray(ec, dtype=np.int32), np.asarray(ew, dtype=np.float64))


def first_upward_crossing(t, v, threshold):
    """Time at which the sampled trace v(t) first goes from below `threshold` to at or above it, linearly interpolated between the
    two samples; NaN if it never does."""
    t, v = np.asarray(t, dtype=np.float64), np.asarray(v, dtype=np.float64)
    k = np.nonzero((v[:-1] < threshold) & (v[1:] >= threshold))[0]
    if not len(k):
        return float("nan")
    k = int(k[0])
    return float(t[k] + (threshold - v[k]) / (v[k + 1] - v[k]) * (t[k + 1] - t[k]))


def _tag_model(models):
    return {int(m.tag): k for k, m in enumerate(models)}


def state_weights_global(mesh, facet_tags, set_facets, models, names):
    """Per (set, state name), in channel order: (positions in the set of the facets whose model has the state, their area weights
    renormalised over exactly those facets).  Decided by the facets' surface tags (models[k].tag) on the global tables, so every rank
    of a partitioned run gets the same answer; ValueError naming the set and the state when no facet of the set has it."""
    by_tag = _tag_model(models)
    has = [{q: model_has_state(m.ode, q) for q in names} for m in models]
    ft = np.asarray(facet_tags)
    out = []
    for s, facets in enumerate(set_facets):
        facets = np.asarray(facets, dtype=np.int64)
        areas = facet_areas(mesh, facets)
        k_of = np.asarray([by_tag.get(int(t), -1) for t in ft[facets]], dtype=np.int64)
        for q in names:
            keep = np.nonzero([k >= 0 and has[k][q] for k in k_of])[0]
            if not len(keep):
                raise ValueError("membrane set %d: no facet of the set belongs to a membrane model with a state '%s'" % (s, q))
            out.append((keep, areas[keep] / areas[keep].sum()))
    return out


class LocalTables:
    """One rank's part of a global recorder's tables (`localize_tables`)."""


def localize_tables(rec, loc):
    """The tables of the global recorder `rec` (built on the global mesh, membrane sets resolved) as rank `loc.rank` records them;
    `loc` is the rank's partition.LocalMesh.  Pure host work from the global mesh and the partition, the same on every rank.
      point_owner [n_points]   owning rank of every probe = owner of its containing cell
      point_cells [n_points]   local cell id, -1 for a probe another rank owns
      facet_owner(f)           owning rank of global membrane facets = owner of facet_cells[f, 0] (amg.Dist0Space.facet_owner)
      set_facets / set_weights / set_index   per set the owned facets (local ids, set order), their GLOBAL weights and their positions
                               in the global set; a set may be empty here
      region, vol [nc_local]   region id and volume of the local cells (the device counts the owned ones); inv_rvol [n_regions] =
                               1 / global region volume; region_volume_owned [n_regions]
      map_facets / map_pos     owned map facets (local ids) and their positions in rec.map_facets
      facet_local(f)           local ids of global facets, -1 = not on this rank"""
    mesh, part, rank = rec.mesh, loc.part, int(loc.rank)
    if mesh is not part.mesh and mesh.num_cells() != part.mesh.num_cells():
        raise ValueError("localize_tables: the recorder was not built on the partition's global mesh")
    if rec.set_facets is None:
        raise ValueError("localize_tables: the membrane sets are not resolved yet (membrane_tags)")
    T = LocalTables()
    T.rank, T.world = rank, int(part.world)
    owner = np.asarray(part.owner)
    first_cell = np.asarray(mesh.facet_cells)[:, 0]
    f_g2l = np.full(mesh.num_facets(), -1, dtype=np.int64)
    f_g2l[loc.facets_global] = np.arange(len(loc.facets_global))
    T.facet_owner = lambda f: owner[first_cell[np.asarray(f, dtype=np.int64)]]
    T.facet_local = lambda f: f_g2l[np.asarray(f, dtype=np.int64)]
    # probes
    T.point_owner = owner[rec.point_cells].astype(np.int64) if rec.n_points else np.zeros(0, dtype=np.int64)
    T.point_cells = np.where(T.point_owner == rank, loc.g2l[rec.point_cells], -1).astype(np.int64) if rec.n_points \
        else np.zeros(0, dtype=np.int64)
    assert ((T.point_cells < loc.nc_owned)).all()
    # membrane sets
    T.set_facets, T.set_weights, T.set_index = [], [], []
    for f, w in zip(rec.set_facets, rec.set_weights):
        mine = np.nonzero(T.facet_owner(f) == rank)[0]
        lf = f_g2l[f[mine]]
        assert (lf >= 0).all()
        T.set_index.append(mine)
        T.set_facets.append(lf)
        T.set_weights.append(np.asarray(w, dtype=np.float64)[mine])
    # regions
    T.region = np.ascontiguousarray(rec.region[loc.cells_global], dtype=np.uint8)
    T.vol = np.ascontiguousarray(rec.vol[loc.cells_global], dtype=np.float64)
    rvol = np.asarray([rec.vol[rec.region == r].sum() for r in range(rec.n_regions)], dtype=np.float64)
    T.inv_rvol = np.where(rvol > 0.0, 1.0 / np.where(rvol > 0.0, rvol, 1.0), 0.0)
    reg_own, vol_own = T.region[:loc.nc_owned], T.vol[:loc.nc_owned]
    T.region_volume_owned = np.asarray([vol_own[reg_own == r].sum() for r in range(rec.n_regions)], dtype=np.float64)
    # map
    if rec.map_facets is not None:
        T.map_pos = np.nonzero(T.facet_owner(rec.map_facets) == rank)[0].astype(np.int64)
        T.map_facets = f_g2l[rec.map_facets[T.map_pos]]
        assert (T.map_facets >= 0).all()
    else:
        T.map_pos = T.map_facets = None
    return T


def state_entries_local(rec, T, models):
    """This rank's entry lists of the state channels (knp_rec_add_states_part): of every global channel (`state_weights_global`) the
    facets the rank owns, with the global weights.  models: the rank's membrane models (local facet ids, `tag`)."""
    by_tag = _tag_model(models)
    chans = state_weights_global(rec.mesh, rec.facet_tags, rec.set_facets, models, rec.state_names)
    ptr, eh, er, ec, ew = [0], [], [], [], []
    n_names = len(rec.state_names)
    for ch, (keep, w) in enumerate(chans):
        f = rec.set_facets[ch // n_names][keep]
        q = rec.state_names[ch % n_names]
        for i in np.nonzero(T.facet_owner(f) == T.rank)[0]:
            m = models[by_tag[int(rec.facet_tags[f[i]])]]
            lf = int(T.facet_local(f[i]))
            mf = np.asarray(m.facets, dtype=np.int64)
            r = int(np.searchsorted(mf, lf))
            if r >= len(mf) or mf[r] != lf:
                raise KnpError("membrane_states: facet %d has no row in the state table of membrane tag %s on rank %d" % (int(f[i]), m.tag, T.rank))
            eh.append(int(m.handle)); er.append(r); ec.append(int(m.ode.state_indices(q))); ew.append(float(w[i]))
        ptr.append(len(eh))
    return (np.asarray(ptr, dtype=np.int64), np.asarray(eh, dtype=np.int32), np.asarray(er, dtype=np.int64),
            np.asarray(ec, dtype=np.int32), np.asarray(ew, dtype=np.float64))


MAP_FIELDS = ("activation_time", "repolarisation_time", "peak", "peak_time", "n_activations")


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
    membrane_states  names of ODE states (as the membrane models declare them), averaged over every membrane set; the device tables
                  follow with `attach_states(models)` once the membrane models exist
    membrane_map  dict(threshold=0.0, repolarisation=None, tags=None): per-facet activation map, in the units of phi_M;
                  repolarisation None = the threshold, tags None = every membrane facet, else the facets with those surface tags
    local_mesh    partitioned run: this rank's partition.LocalMesh; mesh, tags, points, facet ids and regions are then the GLOBAL
                  ones, every rank makes the same call with the same capacity, and the results are the global ones on every rank.
                  Reading is then COLLECTIVE -- `flush`, `rows` and every property derived from it (`t`, `points`, `membrane`,
                  `regions`), `membrane_map`, `conduction_velocity` and `save` must be called by all ranks at the same point
    """

    def __init__(self, mesh, cell_tags, facet_tags, degree, ion_names, points=None, membrane_sets=None, regions=True, capacity=256,
                 point_tags=None, membrane_tags=None, membrane_states=None, membrane_map=None, local_mesh=None):
        self.mesh = mesh
        self.local_mesh = local_mesh
        self.local = None               # LocalTables of a partitioned run, built by attach
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
        self.state_names = [str(q) for q in membrane_states] if membrane_states else []
        if len(set(self.state_names)) != len(self.state_names) or set(self.state_names) & set(self.channel_names()[1]):
            raise ValueError("membrane_states must be distinct and differ from the other membrane channels")
        if self.state_names and not self._set_spec:
            raise ValueError("membrane_states need at least one membrane set")
        self._states_on_device = False
        self._map_spec = None
        self.map_facets = None
        if membrane_map is not None:
            spec = dict(threshold=0.0, repolarisation=None, tags=None)
            unknown = set(membrane_map) - set(spec)
            if unknown:
                raise ValueError("membrane_map: unknown key %s" % sorted(unknown)[0])
            spec.update(membrane_map)
            if spec["repolarisation"] is None:
                spec["repolarisation"] = spec["threshold"]
            spec["threshold"], spec["repolarisation"] = float(spec["threshold"]), float(spec["repolarisation"])
            if not (np.isfinite(spec["threshold"]) and np.isfinite(spec["repolarisation"])):
                raise ValueError("membrane_map: threshold and repolarisation must be finite")
            self._map_spec = spec
        self._armed = False
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
        if self._map_spec is not None:
            tags = self._map_spec["tags"]
            if tags is None:
                sel = mem
            else:
                tags = [int(x) for x in np.atleast_1d(tags)]
                bad = [x for x in tags if x not in [int(y) for y in membrane_tags]]
                if bad:
                    raise ValueError("membrane_map: the facets of tag %d are not membrane facets" % bad[0])
                sel = mem[np.isin(self.facet_tags[mem], tags)]
            if not len(sel):
                raise ValueError("membrane_map: the selection holds no membrane facet")
            self.map_facets = np.asarray(sel, dtype=np.int64)

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

    def attach(self, dev, membrane_tags=None, models=None):
        """Create the device recorder on `dev` (a knpemidg._abi.Device without ghost cells).  models: the membrane models, for the
        state channels; they may follow later through `attach_states`."""
        if self.set_facets is None:
            self.resolve_sets(membrane_tags if membrane_tags is not None else [])
        if self.local_mesh is not None:
            # every host-side decision that can fail is taken on the global tables first, identically on every rank, so that no rank
            # leaves its peers waiting in a collective
            if self.state_names and models is not None:
                state_weights_global(self.mesh, self.facet_tags, self.set_facets, models, self.state_names)
            T = self.local = localize_tables(self, self.local_mesh)
            ptr = np.concatenate([[0], np.cumsum([len(f) for f in T.set_facets])]).astype(np.int64)
            sf = np.concatenate(T.set_facets) if T.set_facets else np.zeros(0, dtype=np.int64)
            sw = np.concatenate(T.set_weights) if T.set_facets else np.zeros(0)
            self.n_channels = dev.rec_create(self.capacity, T.point_cells, self.point_w, ptr, sf, sw, self.n_regions, T.region, T.vol,
                                             inv_rvol=T.inv_rvol)
        else:
            ptr = np.concatenate([[0], np.cumsum([len(f) for f in self.set_facets])]).astype(np.int64)
            sf = np.concatenate(self.set_facets) if self.set_facets else np.zeros(0, dtype=np.int64)
            sw = np.concatenate(self.set_weights) if self.set_facets else np.zeros(0)
            self.n_channels = dev.rec_create(self.capacity, self.point_cells, self.point_w, ptr, sf, sw, self.n_regions, self.region, self.vol)
        n_ions = len(self.ion_names)
        self.n_base = self.n_points * (n_ions + 1) + self.n_sets * (1 + 2 * n_ions) + self.n_regions * (n_ions + 1)
        assert self.n_channels == self.n_base
        self.dev = dev
        self._waiting = 0
        self._states_on_device = False
        if self._map_spec is not None:
            if self.local is not None:
                dev.rec_add_map(self.local.map_facets, self._map_spec["threshold"], self._map_spec["repolarisation"],
                                positions=self.local.map_pos, n_global=len(self.map_facets))
            else:
                dev.rec_add_map(self.map_facets, self._map_spec["threshold"], self._map_spec["repolarisation"])
            self._armed = False
        if self.state_names and models is not None:
            self.attach_states(models)

    def attach_states(self, models):
        """Build and upload the entry lists of the state channels from the membrane models (`state_entries`); right after `attach`,
        before the first sample."""
        if not self.state_names or self._states_on_device:
            return
        if self.dev is None:
            raise KnpError("the recorder is not attached to a device context yet")
        for m in models:
            if getattr(m, "handle", None) is None:
                raise KnpError("membrane_states: the state tables of membrane tag %s are not on the device (KNP_HOST_ODE=1, or a model "
                               "without a device implementation)" % getattr(m, "tag", "?"))
        if self.local is not None:
            self.state_entry_lists = state_entries_local(self, self.local, models)
            self.n_channels = self.dev.rec_add_states(*self.state_entry_lists, part=True)
        else:
            areas = [facet_areas(self.mesh, f) for f in self.set_facets]
            self.state_entry_lists = state_entries(self.set_facets, areas, models, self.state_names)
            self.n_channels = self.dev.rec_add_states(*self.state_entry_lists)
        assert self.n_channels == self.n_base + self.n_sets * len(self.state_names)
        self._states_on_device = True

    def arm(self, t0):
        """Arm the membrane map at time t0: peak = previous value = phi_M now, no crossing seen yet.  The solver's time loops call
        it; call it yourself when stepping by hand.  Without a map: nothing."""
        if self._map_spec is None:
            return
        if self.dev is None:
            raise KnpError("the recorder is not attached to a device context yet")
        self.dev.rec_map_arm(float(t0))
        self._armed = True

    # -- sampling -----------------------------------------------------------------
    def sample(self, t):
        """One row at time t (asynchronous).  A full device buffer is read back first: the only synchronisation."""
        if self.dev is None:
            raise KnpError("the recorder is not attached to a device context yet")
        if self.state_names and not self._states_on_device:
            raise KnpError("membrane_states need the membrane models (setup_membrane_model / Recorder.attach_states) before the first sample")
        if self._map_spec is not None and not self._armed:
            raise KnpError("the membrane map is not armed (Recorder.arm(t0))")
        if self._waiting >= self.capacity:
            self.flush()
        self.dev.rec_sample(float(t))
        self._waiting += 1

    def flush(self):
        """Read the waiting rows back.  Partitioned run: the rows are summed over the ranks on the way -- collective."""
        if self.dev is None or not self._waiting:
            return
        t, rows = self.dev.rec_read()
        assert len(t) == self._waiting
        self._t.append(t)
        self._rows.append(rows)
        self._waiting = 0

    # -- checkpoint (Solver.save_checkpoint) ---------------------------------------------
    def host_state(self, prefix):
        """The rows already read back and the host's view of the device buffer; the buffer itself, its row counter and the map
        accumulators travel in the device snapshot (csrc/record.hip), so saving reads nothing back and changes nothing."""
        out = {prefix + "flags": np.asarray([self._waiting, int(self._armed), getattr(self, "n_channels", 0)], dtype=np.int64)}
        if self._rows:
            out[prefix + "rows"] = np.concatenate(self._rows)
            out[prefix + "t"] = np.concatenate(self._t)
        return out

    def load_host_state(self, prefix, arrays):
        flags = arrays.get(prefix + "flags")
        if flags is None or int(flags[2]) != getattr(self, "n_channels", 0):
            raise KnpError("checkpoint: the recorder layout differs (field 'recorder': %s channels in the file, %d here)"
                           % ("no" if flags is None else int(flags[2]), getattr(self, "n_channels", 0)))
        self._waiting, self._armed = int(flags[0]), bool(flags[1])
        self._rows = [np.asarray(arrays[prefix + "rows"], dtype=np.float64)] if prefix + "rows" in arrays else []
        self._t = [np.asarray(arrays[prefix + "t"], dtype=np.float64)] if prefix + "t" in arrays else []

    # -- results ------------------------------------------------------------------
    @property
    def rows(self):
        """All samples so far, [n_steps, n_channels] in the row layout of include/knpemi_hip.h.  Partitioned run: the global rows,
        the same bits on every rank; collective while rows wait on the device (see `flush`)."""
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
        """{name: [n_steps, n_sets]}: phi_M, E_<ion>, I_ch_<ion> and, with membrane_states, one entry per state name."""
        n_ions = len(self.ion_names)
        out = self._block(self.n_points * (n_ions + 1), self.n_sets, self.channel_names()[1])
        if self.state_names and self._states_on_device:
            out.update(self._block(self.n_base, self.n_sets, self.state_names))
        return out

    @property
    def membrane_map(self):
        """The per-facet map as it stands: facets (caller's ids), activation_time, repolarisation_time (NaN = not yet), peak,
        peak_time, n_activations.  Synchronises and reads the device arrays in one transfer.  Partitioned run: the merged global
        map with global facet ids on every rank; collective."""
        if self._map_spec is None:
            raise KnpError("no membrane map was asked for (record(membrane_map=...))")
        if self.dev is None or not self._armed:
            raise KnpError("the membrane map is not armed yet")
        out = {"facets": self.map_facets.copy()}
        out.update(zip(MAP_FIELDS, self.dev.rec_map_read()))
        return out

    def set_centroid(self, s):
        return self.set_weights[s] @ self.mesh.facet_midpoints()[self.set_facets[s]]

    def conduction_velocity(self, set_a, set_b, distance=None, method="map", threshold=None):
        """distance / (t_b - t_a) between two membrane sets (reference: get_velocity, make_figures_rat_neuron.py:613-692).
        method "map": t = area-weighted mean of the map's per-facet activation times over the set (every facet of both sets must be
        in the map).  method "set_mean": t = first upward crossing of `threshold` (default: the map's, else 0) by the recorded
        set-mean phi_M, linearly interpolated between steps -- the reference's definition at sub-step resolution.  distance defaults
        to the distance between the area-weighted centroids.  NaN when either set has not (entirely) activated.  Partitioned run:
        collective (it reads the map or the rows)."""
        if distance is None:
            distance = float(np.linalg.norm(self.set_centroid(set_b) - self.set_centroid(set_a)))
        if method == "map":
            m = self.membrane_map
            pos = {int(f): i for i, f in enumerate(m["facets"])}
            times = []
            for s in (set_a, set_b):
                missing = [int(f) for f in self.set_facets[s] if int(f) not in pos]
                if missing:
                    raise ValueError("membrane set %d: facet %d is not in the membrane map" % (s, missing[0]))
                idx = np.asarray([pos[int(f)] for f in self.set_facets[s]], dtype=np.int64)
                times.append(float(self.set_weights[s] @ m["activation_time"][idx]))
        elif method == "set_mean":
            if threshold is None:
                threshold = self._map_spec["threshold"] if self._map_spec is not None else 0.0
            v = self.membrane["phi_M"]
            times = [first_upward_crossing(self.t, v[:, s], float(threshold)) for s in (set_a, set_b)]
        else:
            raise ValueError("method must be 'map' or 'set_mean'")
        if not np.isfinite(times).all():
            return float("nan")
        return distance / (times[1] - times[0])

    @property
    def regions(self):
        n_ions = len(self.ion_names)
        return self._block(self.n_points * (n_ions + 1) + self.n_sets * (1 + 2 * n_ions), self.n_regions, self.channel_names()[2])

    def save(self, path):
        """/timeseries/t, /timeseries/points/<name>, /timeseries/membrane/<name>, /timeseries/regions/<name> ([n_steps, n_items]) plus
        the probe coordinates and cells, the facets and weights of every membrane set and the region tags; with a map,
        /membrane_map/{facets, activation_time, repolarisation_time, peak, peak_time, n_activations, threshold, repolarisation}.
        Partitioned run: collective; every rank takes part in the reads, rank 0 alone writes the file (the others return None)."""
        import os
        from knpemidg.h5lite import H5Writer
        if self.local_mesh is not None:
            self.flush()
            m_all = self.membrane_map if self._map_spec is not None and self._armed else None
            if int(self.local_mesh.rank) != 0:
                return None
        else:
            m_all = None
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
            if self._map_spec is not None and self._armed:
                m = m_all if m_all is not None else self.membrane_map
                w.write("/membrane_map/facets", m["facets"].astype(np.int64))
                for name in MAP_FIELDS[:4]:
                    w.write("/membrane_map/" + name, m[name])
                w.write("/membrane_map/n_activations", m["n_activations"].astype(np.int64))
                w.write("/membrane_map/threshold", np.asarray([self._map_spec["threshold"]]))
                w.write("/membrane_map/repolarisation", np.asarray([self._map_spec["repolarisation"]]))
        return path
