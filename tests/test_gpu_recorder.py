"""Time-series recorder on the device (csrc/record.hip) against numpy on the fields read back with knp_download, through the
C ABI and through `Solver.record`.  Both sides evaluate the same sums from the same doubles; only the order of summation differs,
hence the project's operator-parity tolerance of 1e-11, taken relative to each channel's scale = the sum of the magnitudes of the
terms the channel adds up (a channel may itself cancel to nearly zero, e.g. the volume mean of a random potential)."""
import os
import sys

import numpy as np
import pytest

import knpemi_oracle as ko
from common import synthetic_state, device_for, push_state, small_3d

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "idealized_geometries"))

TOL = 1e-11


def expected_row(fields, phiM, E, Ich, point_cells, point_w, sets, region, n_regions, vol, wn):
    """(row, scale) in the layout of include/knpemi_hip.h.  fields = [phi, c_0 .. c_{n_sys-1}, c_elim], each [nc, nd] in the caller's
    cell order; E, Ich [n_ions, nf]; sets = [(facets, weights)]."""
    row, scale = [], []

    def add(terms, factor=1.0):
        row.append(terms.sum() * factor)
        scale.append(np.abs(terms).sum() * factor)
    for p in range(len(point_cells)):
        for f in fields:
            add(point_w[p] * f[point_cells[p]])
    for facets, w in sets:
        for f in [phiM] + list(E) + list(Ich):
            add(w * f[facets])
    for r in range(n_regions):
        sel = region == r
        for f in fields[1:]:
            add(vol[sel] * (f[sel] @ wn))
        add(vol[sel] * (fields[0][sel] @ wn), 1.0 / vol[sel].sum())
    return np.asarray(row), np.asarray(scale)


def channel_errors(row, ref, scale):
    """|row - ref| / scale per channel.  A channel whose terms are all exactly zero (scale 0: e.g. the chloride channel current of
    a Hodgkin-Huxley membrane) has to be exactly zero on the device too: any difference there counts as infinite."""
    diff = np.abs(np.asarray(row) - ref)
    out = np.where(diff == 0.0, 0.0, np.inf)
    nz = scale > 0
    out[nz] = diff[nz] / scale[nz]
    return out


def _probe_points(mesh, cell_tags, dev):
    """One probe in every subdomain, one in the first and one in the last cell in device order, one exactly on a vertex."""
    mid = mesh.cell_midpoints()
    pts = [mid[np.nonzero(cell_tags == t)[0][len(np.nonzero(cell_tags == t)[0]) // 2]] for t in np.unique(cell_tags)]
    pts += [mid[dev.cell_order[0]], mid[dev.cell_order[-1]], mesh.coords[mesh.cells[mesh.num_cells() // 3, 1]]]
    return np.asarray(pts)


CASES = {"2D_P1": ("2d", 1), "2D_P2": ("2d", 2), "3D_P1": ("3d", 1), "3D_P2": ("3d", 2)}


@pytest.mark.parametrize("case", list(CASES))
def test_kernels_against_numpy_through_the_abi(hip_lib, case):
    """Every channel of two consecutive samples against numpy.  Membrane sets: all membrane facets, a single facet and a list of
    65 entries (a wave plus one).  The 2D r=0 mesh has 62 membrane facets and small_3d((7, 4, 4)) has 64, so the 65-entry list names
    every membrane facet once and the first ones twice, with random positive weights -- at the ABI a set is a list of (facet, weight)
    pairs, and 65 entries is what makes a second wave of the workgroup take part."""
    from knpemidg import _abi as A
    from knpemidg import recorder as R
    from knpemidg.mesh import make_mesh_2D
    which, p = CASES[case]
    m, s, f = make_mesh_2D(0) if which == "2d" else small_3d((7, 4, 4))
    if which == "3d":
        assert m.num_cells() > 512 and m.num_cells() % 256 != 0       # several region blocks, the last one partial
    pb = ko.build_idealized(m, s.array(), f.array(), p=p, membrane_tags=(1,))
    synthetic_state(pb)
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        rng = np.random.default_rng(11)
        nf, n_ions = m.num_facets(), len(pb.ions)
        dev.upload(A.F_PHI_M, 0.07 * rng.uniform(-1, 1, size=nf))
        dev.upload(A.F_E, 0.1 * rng.uniform(-1, 1, size=(n_ions, nf)))
        dev.upload(A.F_I_CH, 1e-3 * rng.uniform(-1, 1, size=(n_ions, nf)))
        tags = np.asarray(s.array())
        pts = _probe_points(m, tags, dev)
        cells, bary = R.locate_points(m, pts)
        assert dev.cell_rank[cells[len(np.unique(tags))]] == 0 and dev.cell_rank[cells[len(np.unique(tags)) + 1]] == m.num_cells() - 1
        w = R.basis_weights(bary, p)
        mem = R.membrane_facets(m, f.array(), [1])
        assert len(mem) >= 62
        long_set = np.concatenate([mem, mem])[:65]
        sets = []
        for facets in (mem, mem[7:8], long_set):
            a = rng.uniform(0.5, 1.5, size=len(facets))
            sets.append((facets, a / a.sum()))
        region_tags = np.unique(tags)
        region = np.searchsorted(region_tags, tags).astype(np.uint8)
        region[::17] = R.REGION_NONE                                   # some cells outside every region
        vol = R.cell_volumes(m)
        ptr = np.concatenate([[0], np.cumsum([len(fs) for fs, _ in sets])])
        n_ch = dev.rec_create(8, cells, w, ptr, np.concatenate([fs for fs, _ in sets]), np.concatenate([ws for _, ws in sets]),
                              len(region_tags), region, vol)
        assert n_ch == len(pts) * (n_ions + 1) + 3 * (1 + 2 * n_ions) + len(region_tags) * (n_ions + 1)
        wn = R.nodal_integration_weights(m.gdim, p)

        def host():
            nc, nd = m.num_cells(), pb.nd
            c = dev.download(A.F_C).reshape(n_ions - 1, nc, nd)
            fields = [dev.download(A.F_PHI).reshape(nc, nd)] + list(c) + [dev.download(A.F_C_ELIM).reshape(nc, nd)]
            return expected_row(fields, dev.download(A.F_PHI_M), dev.download(A.F_E).reshape(n_ions, nf),
                                dev.download(A.F_I_CH).reshape(n_ions, nf), cells, w, sets, region, len(region_tags), vol, wn)
        dev.rec_sample(0.25)
        ref0, sc0 = host()
        dev.upload(A.F_PHI, 2.0 * pb.phi + 0.01)                       # second row from another state
        dev.rec_sample(0.5)
        ref1, sc1 = host()
        t, rows = dev.rec_read()
        assert list(t) == [0.25, 0.5] and rows.shape == (2, n_ch)
        for k, (ref, sc) in enumerate(((ref0, sc0), (ref1, sc1))):
            err = channel_errors(rows[k], ref, sc)
            print("%s row %d: worst channel error / scale %.2e" % (case, k, err.max()))
            assert (sc > 0).all() and err.max() < TOL, (case, k, int(err.argmax()), err.max())
        assert not np.array_equal(rows[0], rows[1])
        t, rows = dev.rec_read()                                       # emptied by the read
        assert len(t) == 0 and rows.shape == (0, n_ch)
        # a full buffer refuses further samples instead of overwriting rows
        for k in range(8):
            dev.rec_sample(float(k))
        with pytest.raises(A.KnpError, match="-5"):
            dev.rec_sample(8.0)
        t, rows = dev.rec_read()
        assert list(t) == [float(k) for k in range(8)] and all(np.array_equal(rows[k], rows[0]) for k in range(8))
    finally:
        dev.close()


def test_bad_input_is_refused_through_the_abi(hip_lib):
    """A ghost or out-of-range cell, a facet that is no membrane facet, an empty set and a region id >= n_regions: non-zero status
    with a message, no recorder afterwards (so nothing can be launched on the bad tables)."""
    from knpemidg import _abi as A
    from knpemidg import recorder as R
    from knpemidg.partition import Partition
    m, s, f = small_3d((8, 4, 4))
    loc = Partition(m, 2, method="slab").local(0)
    sub_l, surf_l = loc.localize(s, f, (1,))
    pb = ko.build_idealized(loc.mesh, sub_l.array(), surf_l.array(), membrane_tags=(1,))
    dev = device_for(pb, nc_owned=loc.nc_owned)
    try:
        lm = loc.mesh
        nc, no = lm.num_cells(), loc.nc_owned
        assert no < nc
        mem = R.membrane_facets(lm, surf_l.array(), [1])
        mem = mem[(lm.facet_cells[mem] < no).all(axis=1)]
        not_mem = int(np.nonzero(np.asarray(surf_l.array()) == 0)[0][0])
        w1 = np.full((1, 4), 0.25)
        region = np.zeros(nc, dtype=np.uint8)
        vol = R.cell_volumes(lm)
        none = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
        one_set = (np.array([0, 2]), mem[:2], np.array([0.5, 0.5]))

        def refused(msg, *args):
            with pytest.raises(A.KnpError, match=msg):
                dev.rec_create(*args)
            assert dev.lib.knp_rec_channels(dev.ctx) < 0
            with pytest.raises(A.KnpError, match="no recorder"):
                dev.rec_sample(0.0)
        assert dev.cell_rank[no] >= no                                  # ghosts keep their places behind the owned cells
        refused("not an owned cell", 4, [no], w1, *none, 0, None, None)                       # a ghost cell
        bad_cell = np.array([nc + 5])
        with pytest.raises(A.KnpError, match="not an owned cell"):                            # out of range, past the Python permutation
            pc = np.ascontiguousarray(bad_cell, dtype=np.int32)
            sp = np.zeros(1, dtype=np.int64)
            dev._chk(dev.lib.knp_rec_create(dev.ctx, 4, 1, A._p(pc, A._i32p), A._p(w1, A._f64p), 0, A._p(sp, A._i64p), None, None, 0,
                                            None, None), "knp_rec_create")
        refused("not a membrane facet", 4, [], np.zeros((0, 4)), np.array([0, 2]), np.array([mem[0], not_mem]), np.array([0.5, 0.5]),
                0, None, None)
        refused("not a membrane facet", 4, [], np.zeros((0, 4)), np.array([0, 1]), np.array([lm.num_facets()]), np.array([1.0]),
                0, None, None)
        refused("is empty", 4, [], np.zeros((0, 4)), np.array([0, 1, 1]), mem[:1], np.array([1.0]), 0, None, None)
        bad_region = region.copy()
        bad_region[3] = 2
        refused("region id 2", 4, [], np.zeros((0, 4)), *none, 2, bad_region, vol)
        # the same tables without the bad entries are accepted, and region id 255 is not an error
        region[5] = R.REGION_NONE
        assert dev.rec_create(4, [0], w1, *one_set, 2, region, vol) == 4 + 7 + 8
        dev.rec_sample(0.0)
        t, rows = dev.rec_read()
        assert len(t) == 1 and np.isfinite(rows).all()
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# through the solver
# ---------------------------------------------------------------------------------------------------------------------
class CountingLib:
    """The library with its recorder entry points counted."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("knp_rec_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


N_STEPS = 6


def _run_3d(capacity, check=False):
    """Six steps of the 3D single-axon solver; capacity None = no recorder.  Returns a dict with the final fields, the recorder's
    output, the counted recorder calls and (check) the host-evaluated rows."""
    from idealized_common import make_solver, solver_parameters, Constant
    from knpemidg import recorder as R
    mt = small_3d((7, 4, 4))
    S = make_solver(dim=3, mesh_tuple=mt, n_axons=1)
    S.dev.lib = lib = CountingLib(S.dev.lib)
    mesh, tags = mt[0], np.asarray(mt[1].array())
    rec = None
    if capacity is not None:
        mid = mesh.cell_midpoints()
        pts = [mid[np.nonzero(tags == 0)[0][10]], mid[np.nonzero(tags == 1)[0][10]], mesh.coords[mesh.cells[100, 2]]]
        box = (np.array([2.0e-6, 0.05e-6, 0.05e-6]), np.array([3.5e-6, 0.35e-6, 0.11e-6]))
        rec = S.record(points=pts, membrane_sets=[box, R.membrane_facets(mesh, mt[2].array(), [1])], regions=True, capacity=capacity)
    # the measured choice of the EMI smoother depends on timings: fixed here, so that two runs are the same computation
    S._unpack_solver_params(solver_parameters(3, 0, emi_dg_chebyshev=True))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    t = Constant(0.0)
    times, host_rows, host_scale = [], [], []
    for k in range(N_STEPS):
        S.step_membrane_models(k)
        S.solve_for_time_step(k, t)
        times.append(float(t))
        if check:
            fields = [S.phi.array()] + list(S.c.array()) + [S.ion_list[-1]['c'].array()]
            E = [ion['E'].array() for ion in S.ion_list]
            Ich = [S.mem_models[0]['I_ch_k'][ion['name']].array() for ion in S.ion_list]
            sets = list(zip(rec.set_facets, rec.set_weights))
            row, sc = expected_row(fields, S.phi_M_prev_PDE.array(), E, Ich, rec.point_cells, rec.point_w, sets, rec.region, rec.n_regions,
                                   rec.vol, R.nodal_integration_weights(3, 1))
            host_rows.append(row)
            host_scale.append(sc)
    out = {"phi": S.phi.array(), "c": S.c.array(), "times": times, "host_rows": host_rows, "host_scale": host_scale}
    if rec is not None:
        out.update(t=rec.t.copy(), rows=rec.rows.copy(), points=rec.points, membrane=rec.membrane, regions=rec.regions,
                   region_tags=rec.region_tags, n_sets=rec.n_sets)
    out["calls"] = dict(lib.calls)
    S.dev.close()
    return out


@pytest.fixture(scope="module")
def runs(hip_lib):
    return {"cap4": _run_3d(4, check=True), "cap64": _run_3d(64), "none": _run_3d(None)}


def test_solver_rows_match_the_host_at_every_step(runs):
    r = runs["cap4"]
    assert r["rows"].shape[0] == N_STEPS and list(r["t"]) == r["times"]
    for k in range(N_STEPS):
        err = channel_errors(r["rows"][k], r["host_rows"][k], r["host_scale"][k])
        print("step %d: worst channel error / scale %.2e" % (k, err.max()))
        assert err.max() < TOL, (k, int(err.argmax()), err.max())
    assert not np.array_equal(r["rows"][0], r["rows"][-1])
    # the named views are slices of the same rows
    assert r["points"]["phi"].shape == (N_STEPS, 3) and r["membrane"]["phi_M"].shape == (N_STEPS, 2)
    assert r["regions"]["phi_mean"].shape == (N_STEPS, 2) and r["region_tags"] == [0, 1]
    assert np.array_equal(r["points"]["K"][:, 1], r["rows"][:, 4 + 1]) and np.array_equal(r["membrane"]["E_K"][:, 0], r["rows"][:, 12 + 1])
    assert np.array_equal(r["regions"]["Na"][:, 1], r["rows"][:, 12 + 14 + 4 + 2])
    # capacity 4: one read when the buffer is full, one at the end; nothing else synchronises
    assert r["calls"] == {"knp_rec_create": 1, "knp_rec_channels": 1, "knp_rec_sample": N_STEPS, "knp_rec_read": 2}


def test_buffer_capacity_does_not_change_the_rows(runs):
    a, b = runs["cap4"], runs["cap64"]
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["t"], b["t"])
    assert b["calls"]["knp_rec_read"] == 1


def test_two_fresh_solvers_give_the_same_bits(hip_lib, runs):
    again = _run_3d(64)
    assert np.array_equal(again["rows"], runs["cap64"]["rows"]) and np.array_equal(again["t"], runs["cap64"]["t"])


def test_no_recorder_no_change(runs):
    a, n = runs["cap4"], runs["none"]
    assert np.array_equal(a["phi"], n["phi"]) and np.array_equal(a["c"], n["c"])
    assert n["calls"] == {}


def test_partitioned_solver_refuses_a_recorder(hip_lib):
    from idealized_common import make_solver
    from knpemidg import _abi as A
    S = make_solver(dim=3, mesh_tuple=small_3d((7, 4, 4)), n_axons=1)
    try:
        S.nc_owned = S.mesh.num_cells() - 1            # what distribute_solver sets on a partition
        with pytest.raises(A.KnpError, match="partitioned"):
            S.record(regions=True)
    finally:
        S.dev.close()


def test_timeseries_file(hip_lib, tmp_path):
    from idealized_common import make_solver, solver_parameters, Constant
    from knpemidg.h5lite import H5File
    from knpemidg import recorder as R
    S = make_solver(dim=2, resolution=0)
    mesh, tags = S.mesh, np.asarray(S.subdomains.array())
    mid = mesh.cell_midpoints()
    pts = [mid[np.nonzero(tags == 0)[0][3]], mid[np.nonzero(tags == 1)[0][3]]]
    mem = R.membrane_facets(mesh, S.surfaces.array(), [1])
    rec = S.record(points=pts, membrane_sets=[mem[:5]], regions=True)
    prefix = str(tmp_path) + os.sep + "run_"
    S.solve_system_active(3e-4, Constant(0.0), solver_parameters(2, 0), filename=prefix)
    path = prefix + "timeseries.h5"
    assert os.path.exists(path) and not os.path.exists(prefix + "results.h5")
    h = H5File(path)
    assert rec.t.shape == (3,) and np.array_equal(h.read("timeseries/t"), rec.t)
    for group, data in (("points", rec.points), ("membrane", rec.membrane), ("regions", rec.regions)):
        for name, a in data.items():
            got = h.read("timeseries/%s/%s" % (group, name))
            assert got.shape == a.shape and a.shape[0] == 3 and np.array_equal(got, a), (group, name)
    assert set(rec.points) == {"phi", "K", "Cl", "Na"} and set(rec.regions) == {"K", "Cl", "Na", "phi_mean"}
    assert set(rec.membrane) == {"phi_M", "E_K", "E_Cl", "E_Na", "I_ch_K", "I_ch_Cl", "I_ch_Na"}
    assert np.array_equal(h.read("probes/coordinates"), np.asarray(pts)) and np.array_equal(h.read("membrane_sets/set_0/facets"), mem[:5])
    assert np.isfinite(rec.rows).all() and np.abs(rec.membrane["phi_M"]).max() > 0.01
    S.dev.close()
