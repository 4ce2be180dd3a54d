"""Derived grid quantities on the device (csrc/grid.hip: k_grid_sample_derived) against their host statement
(GridSpec.sample_derived, which tests/test_grid_flux_host.py pins to analysis): electric field, flux and diffusive flux of every ion
and the current density in one grid, every component within 1e-11 kappa (1 + |p| / diam) S of the host value evaluated with the
host's owners and lambda (grid_flux_cases.vector_bound), on grids in generic position and on grids with points on facets, edges and
vertices; then the tag filter on the membrane, mixed and derived-only grids, fp32 frames, the refusals of knp_grid_create_derived
and the frames a time loop writes."""
import gc
import os
import sys

import numpy as np
import pytest

import grid_cases as G
import grid_flux_cases as GF
from common import device_for, push_state, set_params_of
from knpemidg.grid import GridSpec

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples", "idealized_geometries"))


@pytest.fixture(scope="module", autouse=True)
def _release_shared_references():
    """As in test_gpu_grid.py: the shared meshes and host references are released when the module ends."""
    yield
    for cached in (G.mesh_tuple, G.spec, G.located, G.candidates):
        cached.cache_clear()
    gc.collect()


def _frame(dev, s, fields, quantities, dtype=np.float64):
    """(handle, owner, nodal planes [n_fields, npts], vectors [n_quantities, npts, d], the raw frame) of one grid, sampled once."""
    h = dev.grid_create(s.lo, s.h, s.shape, fields, tol=s.tol, tags=s.tags, f32=dtype == np.float32, derived=quantities)
    owner, _ = dev.grid_points(h, s.npts)
    dev.grid_sample(h)
    d, nf, nq = s.dim, len(fields), len(quantities)
    a = dev.grid_fetch(h, nf + d * nq, s.npts, dtype)
    return h, owner, a[:nf], a[nf:].reshape(nq, d, s.npts).transpose(0, 2, 1), a


def _problem(name, p):
    """grid_cases' problem with its discontinuous synthetic state and D differing by subdomain; (pb, names, quantities, D)."""
    pb = G.problem(name, p)
    D = GF.scale_problem(pb)
    names, quantities = GF.all_quantities([ion["name"] for ion in pb.ions])
    return pb, names, quantities, D


def _replica(pb, mesh, s, quantities, D, owner, bary, fields=None):
    fields = G.nodal_fields(pb) if fields is None else fields
    z = np.array([ion["z"] for ion in pb.ions], dtype=np.float64)
    return s.sample_derived(mesh, quantities, fields[0], fields[1:], z, D, pb.psi, pb.F, pb.p, owner, bary)


def _check(mesh, s, owner, got, want, scale):
    found = owner >= 0
    assert np.array_equal(np.isnan(got), np.broadcast_to(~found[None, :, None], got.shape))
    return GF.worst_ratio(got, want, GF.vector_bound(mesh, s.points(), owner, scale), found)


@pytest.mark.parametrize("name,p", [("2d", 1), ("2d", 2), ("3d", 1), ("3d", 2), ("emix", 1)])
def test_generic_position(hip_lib, name, p):
    """37x29 / 23x19x17 in generic position, the discontinuous synthetic state, every quantity of every ion in one grid
    (2 n_ions + 2 = 8 quantities): NaN exactly where no cell owns the point, every component within the bound of the host value."""
    mesh = G.mesh_tuple(name)[0]
    s = G.spec(name, "generic")
    h_owner, h_bary = G.located(name, "generic")[:2]
    pb, names, quantities, D = _problem(name, p)
    assert len(np.unique(D[0])) >= 2 and len(quantities) == 2 * len(pb.ions) + 2
    want, scale = _replica(pb, mesh, s, quantities, D, h_owner, h_bary)
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        _, owner, _, got, _ = _frame(dev, s, [], quantities)
        assert np.array_equal(owner, h_owner)
        worst = _check(mesh, s, h_owner, got, want, scale)
        print("%s P%d: largest error / bound %.2e" % (name, p, worst))
        assert worst < 1.0
        assert np.abs(got[names.index("current")][h_owner >= 0]).max() > 0.0
    finally:
        dev.close()


@pytest.mark.parametrize("name,p", [("2d", 1), ("2d", 2), ("3d", 1), ("3d", 2)])
def test_points_on_facets_edges_and_vertices(hip_lib, monkeypatch, name, p):
    """The exact grids (33x33, 17x9x9) with affine nodal data phi = a.x + b, c_k = g_k.x + e_k: the points on facets, edges and
    vertices return -a and -D_owner g_k with the D of the cell the lowest-id rule names, and the fluxes built from them; a context
    built with KNP_NO_REORDER=1 gives the same bits in every plane."""
    from knpemidg import _abi as A
    mesh = G.mesh_tuple(name)[0]
    s = G.spec(name, "exact")
    h_owner, h_bary = G.located(name, "exact")[:2]
    assert (h_owner >= 0).all()
    pb, names, quantities, D = _problem(name, p)
    x = GF.node_points(mesh, p)
    L = mesh.coords.max(axis=0) - mesh.coords.min(axis=0)
    d = mesh.gdim
    a = np.array([0.7, -1.3, 2.1])[:d] / L * 0.05
    g = np.array([[1.1, 0.6, -0.8], [-0.9, 1.4, 0.5], [0.4, -1.2, 1.7]])[:, :d] / L * np.array([4.0, 100.0, 12.0])[:, None]
    e = np.array([60.0, 1500.0, 180.0])
    fields = [x @ a + 0.4] + [x @ g[k] + e[k] for k in range(3)]
    assert all((f > 0).all() for f in fields[1:])
    pts = s.points()
    z = np.array([ion["z"] for ion in pb.ions], dtype=np.float64)
    Dp = D[:, h_owner]
    closed = np.empty((len(quantities), s.npts, d))
    cur = np.zeros((s.npts, d))
    for k, ion in enumerate(pb.ions):
        flux = -Dp[k][:, None] * (g[k] + z[k] * pb.psi * (pts @ g[k] + e[k])[:, None] * a)
        closed[names.index("diffusive_flux_" + ion["name"])] = -Dp[k][:, None] * g[k]
        closed[names.index("flux_" + ion["name"])] = flux
        cur += pb.F * z[k] * flux
    closed[names.index("efield")] = -a
    closed[names.index("current")] = cur
    want, scale = _replica(pb, mesh, s, quantities, D, h_owner, h_bary, fields)
    frames = []
    for reorder in (True, False):
        if not reorder:
            monkeypatch.setenv("KNP_NO_REORDER", "1")
        dev = device_for(pb)
        try:
            assert np.array_equal(dev.cell_order, np.arange(mesh.num_cells())) == (not reorder)
            push_state(dev, pb)
            dev.upload(A.F_PHI, fields[0])
            dev.upload(A.F_C, np.stack(fields[1:3]))
            dev.upload(A.F_C_ELIM, fields[3])
            _, owner, _, got, raw = _frame(dev, s, [], quantities)
            assert np.array_equal(owner, h_owner)
            frames.append((got, raw))
        finally:
            dev.close()
    got = frames[0][0]
    r_host = _check(mesh, s, h_owner, got, want, scale)
    r_closed = _check(mesh, s, h_owner, got, closed, scale)
    print("%s P%d: largest error / bound %.2e (host), %.2e (closed form)" % (name, p, r_host, r_closed))
    assert r_host < 1.0 and r_closed < 1.0
    assert frames[0][1].tobytes() == frames[1][1].tobytes()


def test_tags_give_the_intracellular_side_on_the_membrane(hip_lib):
    """33x9x9 on the 3D mesh with tags=(1,): the points on the membrane carry the intracellular gradient and D.  On the host
    first: the filtered and the unfiltered replica differ in at least one point that both own; then the device against the replica
    under the same filter."""
    mesh, sub, _ = G.mesh_tuple("3d")
    tags = np.asarray(sub.array()).astype(np.int64)
    lo, hi = G.exact_bounds(mesh)
    vol, ics = GridSpec(3, lo, hi, (33, 9, 9)), GridSpec(3, lo, hi, (33, 9, 9), tags=(1,))
    o_all, b_all = vol.locate(mesh)
    o_ics, b_ics = ics.locate(mesh, tags)
    pb, names, quantities, D = _problem("3d", 1)
    w_all, _ = _replica(pb, mesh, vol, quantities, D, o_all, b_all)
    w_ics, scale = _replica(pb, mesh, ics, quantities, D, o_ics, b_ics)
    both = (o_all >= 0) & (o_ics >= 0)
    moved = both & (o_all != o_ics)
    assert moved.sum() == 16 and (tags[o_all[moved]] == 0).all() and (tags[o_ics[moved]] == 1).all()
    assert (np.abs(w_all[:, moved] - w_ics[:, moved]) > GF.vector_bound(mesh, ics.points(), o_ics, scale)[:, moved]).any()
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        _, owner, _, got, _ = _frame(dev, ics, [], quantities)
        assert np.array_equal(owner, o_ics)
        worst = _check(mesh, ics, o_ics, got, w_ics, scale)
        _, owner_all, _, got_all, _ = _frame(dev, vol, [], quantities)
        assert np.array_equal(owner_all, o_all)
        print("3d P1 tags=(1,): largest error / bound %.2e" % worst)
        assert worst < 1.0
        assert not np.array_equal(got[:, moved], got_all[:, moved])
        same = both & (o_all == o_ics)
        assert np.array_equal(got[:, same], got_all[:, same])
    finally:
        dev.close()


def test_mixed_derived_only_and_fp32_grids(hip_lib):
    """(phi, K, efield, flux_K, current): the nodal planes are the bytes of a nodal-only grid on the same state; current equals
    F sum z_k flux_k of the same frame within the bound; a grid without nodal fields works and gives the same bits; the fp32
    frame is the fp64 frame rounded; the checkpoint layout does not change."""
    from knpemidg import _abi as A
    mesh = G.mesh_tuple("3d")[0]
    s = G.spec("3d", "generic")
    h_owner, h_bary = G.located("3d", "generic")[:2]
    found = h_owner >= 0
    pb, names, quantities, D = _problem("3d", 2)
    z = np.array([ion["z"] for ion in pb.ions], dtype=np.float64)
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        table0, bytes0 = dev.state_describe()
        mixed = [(A.GD_EFIELD, -1), (A.GD_FLUX, 0), (A.GD_CURRENT, -1)]
        h_mix, owner, nodal, vec, raw = _frame(dev, s, [0, 1], mixed)
        h_nod = dev.grid_create(s.lo, s.h, s.shape, [0, 1])
        dev.grid_sample(h_nod)
        assert dev.grid_fetch(h_nod, 2, s.npts).tobytes() == nodal.tobytes()
        # current against the fluxes of one frame
        fluxes = [(A.GD_FLUX, k) for k in range(len(pb.ions))] + [(A.GD_CURRENT, -1)]
        h_all, _, none, vf, raw_only = _frame(dev, s, [], fluxes)
        assert none.shape == (0, s.npts)
        total = sum(pb.F * z[k] * vf[k] for k in range(len(pb.ions)))
        _, scale = _replica(pb, mesh, s, [(A.GD_CURRENT, -1)], D, h_owner, h_bary)
        bound = GF.vector_bound(mesh, s.points(), h_owner, scale)
        worst = GF.worst_ratio(vf[-1:], total[None], bound, found)
        print("current against F sum z_k flux_k: largest error / bound %.2e" % worst)
        assert worst < 1.0 and np.abs(vf[-1][found]).max() > 0.0
        # the same quantity has the same bits whatever else the grid holds
        assert vec[1].tobytes() == vf[0].tobytes() and vec[2].tobytes() == vf[-1].tobytes()
        # fp32
        h32, _, n32, v32, raw32 = _frame(dev, s, [0, 1], mixed, dtype=np.float32)
        assert raw32.dtype == np.float32 and np.isnan(raw32).any() and np.array_equal(raw32, raw.astype(np.float32), equal_nan=True)
        table1, bytes1 = dev.state_describe()
        assert bytes1 == bytes0 and table1.tobytes() == table0.tobytes()
        t = dev.grid_timing(h_mix)
        assert len(t) == 4 and all(np.isfinite(v) and v >= 0.0 for v in t) and t[2] > 0.0
    finally:
        dev.close()


def test_refusals_leave_the_context_working(hip_lib):
    """A bad kind, ion = n_ions, ion = -1, nothing selected, too many quantities and a context without parameters are refused with
    their messages; after each a valid create and sample works; the ninth grid is still refused."""
    from knpemidg import _abi as A
    s = G.spec("2d", "generic")
    owner = G.located("2d", "generic")[0]
    pb, names, quantities, D = _problem("2d", 1)
    n_ions = len(pb.ions)

    def works(dev):
        h, o, nodal, vec, _ = _frame(dev, s, [0], [(A.GD_EFIELD, -1), (A.GD_FLUX, n_ions - 1)])
        assert np.array_equal(o, owner) and np.array_equal(np.isnan(vec[1, :, 0]), owner < 0) and np.isfinite(nodal[0][owner >= 0]).all()
        dev.grid_destroy(h)

    bare = A.Device(pb.mesh, pb.cell_tags, pb.facet_tags, pb.membrane_tags, n_ions, degree=pb.p)
    try:
        with pytest.raises(A.KnpError, match="knp_set_params"):
            bare.grid_create(s.lo, s.h, s.shape, [0], derived=[(A.GD_EFIELD, -1)])
        h = bare.grid_create(s.lo, s.h, s.shape, [0])                 # a nodal grid needs no parameters, as before
        bare.grid_destroy(h)
        set_params_of(bare, pb)
        push_state(bare, pb)
        works(bare)
    finally:
        bare.close()
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        table0, bytes0 = dev.state_describe()
        too_many = quantities + [(A.GD_EFIELD, -1)]
        assert len(too_many) == 2 * n_ions + 3
        for what, fields, derived in (("unknown kind", [0], [(4, 0)]), ("unknown kind", [0], [(-1, 0)]), ("outside 0", [0], [(A.GD_FLUX, n_ions)]),
                                      ("outside 0", [], [(A.GD_FLUX_DIFFUSIVE, -1)]), ("between 1 and n_ions", [], []),
                                      ("at most 2 n_ions", [0], too_many), ("field id", [n_ions + 1], [(A.GD_CURRENT, -1)])):
            with pytest.raises(A.KnpError, match=what):
                dev.grid_create(s.lo, s.h, s.shape, fields, derived=derived)
            works(dev)
        table1, bytes1 = dev.state_describe()
        assert bytes1 == bytes0 and table1.tobytes() == table0.tobytes()
        handles = [dev.grid_create(s.lo, s.h, s.shape, [], derived=[(A.GD_CURRENT, -1)]) for _ in range(8)]
        assert sorted(handles) == list(range(8))
        with pytest.raises(A.KnpError, match="at most 8"):
            dev.grid_create(s.lo, s.h, s.shape, [], derived=[(A.GD_EFIELD, -1)])
        dev.grid_sample(handles[5])
        assert np.array_equal(np.isnan(dev.grid_fetch(handles[5], 2, s.npts)[0]), owner < 0)
    finally:
        dev.close()


def _run(tmp_path, monkeypatch, with_grid):
    from idealized_common import Constant, make_solver, solver_parameters
    from knpemidg import _abi as A
    monkeypatch.setenv("KNP_NO_AMG", "1")
    monkeypatch.setenv("KNP_AMG_SERIAL_SETUP", "1")          # no helper process outlives this test with its settings (test_gpu_grid.py)
    sp = solver_parameters(3, 0, emi_dg_chebyshev=True)
    S = make_solver(dim=3, resolution=0, n_axons=4)
    g = None
    if with_grid:
        lo, hi = G.generic_bounds(S.mesh)
        g = S.record_grid(lo, hi, (13, 7, 5), fields=("phi", "efield", "flux_K", "current"), every=2)
    out = str(tmp_path / ("with" if with_grid else "without")) + "/"
    S.solve_system_active(6 * 1e-4, Constant(0.0), sp, filename=out if with_grid else None)
    state = (S.dev.download(A.F_PHI).tobytes(), S.dev.download(A.F_C).tobytes(), S.dev.download(A.F_C_ELIM).tobytes())
    last = {f: np.array(v) for f, v in g.sample().items()} if with_grid else None
    cells = g.cells.copy() if with_grid else None
    S.dev.close()
    return out, state, last, cells


def test_frames_of_a_time_loop(hip_lib, tmp_path, monkeypatch):
    """Idealized 3D at resolution 0, 6 steps, record_grid(fields=(phi, efield, flux_K, current), every=2, shape=(13, 7, 5)): frame 0
    for the starting state and three frames of the loop (steps 2, 4, 6),
    with [5, 7, 13] and [5, 7, 13, 3] datasets, the last one the bits of sampler.sample() after the loop, finite inside,
    NaN outside, a nonzero current, Vector attributes in the sidecar; phi and c after the loop are the bytes of the same run
    without any grid."""
    from knpemidg.h5lite import H5File
    from knpemidg import setup_worker
    idle = len(setup_worker._IDLE)
    out, state, last, cells = _run(tmp_path, monkeypatch, True)
    _, state0, _, _ = _run(tmp_path, monkeypatch, False)
    assert state == state0
    assert sorted(os.listdir(out)) == ["grid.h5", "grid.xdmf"]
    h = H5File(out + "grid.h5")
    assert list(h.read("/step")) == [0, 2, 4, 6]
    inside = cells >= 0
    assert cells.shape == (5, 7, 13) and inside.any() and (~inside).any()
    for n in range(4):
        a = h.read("/phi/vector_%d" % n)
        assert a.shape == (5, 7, 13) and a.dtype == np.float64 and np.array_equal(np.isnan(a), ~inside)
        for f in ("efield", "flux_K", "current"):
            v = h.read("/%s/vector_%d" % (f, n))
            assert v.shape == (5, 7, 13, 3) and v.dtype == np.float64
            assert np.isfinite(v[inside]).all() and np.isnan(v[~inside]).all()
    assert h.read("/phi/vector_3").tobytes() == last["phi"].tobytes()
    for f in ("efield", "flux_K", "current"):
        assert last[f].shape == (5, 7, 13, 3) and h.read("/%s/vector_3" % f).tobytes() == np.ascontiguousarray(last[f]).tobytes()
    assert np.abs(last["current"][inside]).max() > 0.0
    text = open(out + "grid.xdmf").read()
    assert text.count('Name="current" AttributeType="Vector"') == 4 and text.count('Name="phi" AttributeType="Scalar"') == 4
    assert len(setup_worker._IDLE) == idle
