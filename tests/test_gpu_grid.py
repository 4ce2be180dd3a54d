"""Voxel-grid sampler on the device (csrc/grid.hip) against the host path of knpemidg/grid.py, which tests/test_grid_host.py ties
to recorder.locate_points and basis_weights: owners and tags exactly, values within a rounding bound derived for the owning cell
(grid_cases.value_bound), on grids in generic position and on grids whose points sit on facets, edges and vertices; then the tag
filter, slices, fp32 frames, several grids, the frames a time loop writes, the checkpoint layout and the several-ranks refusal."""
import gc
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import grid_cases as G
from common import device_for, push_state, small_3d
from knpemidg.grid import GridSpec

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples", "idealized_geometries"))


@pytest.fixture(scope="module", autouse=True)
def _release_shared_references():
    """The meshes, grids and host references of grid_cases are computed once and shared by the tests of this module; they are
    released when it ends, so that the tests after it find the process as small as they would without this module."""
    yield
    for cached in (G.mesh_tuple, G.spec, G.located, G.candidates):
        cached.cache_clear()
    gc.collect()


def _frame(dev, s, n_fields, dtype=np.float64, **kw):
    """(handle, owner, tag, frame [n_fields, npts]) of a grid with the first n_fields field ids, sampled once."""
    h = dev.grid_create(s.lo, s.h, s.shape, list(range(n_fields)), tol=s.tol, tags=s.tags, f32=dtype == np.float32, **kw)
    owner, tag = dev.grid_points(h, s.npts)
    dev.grid_sample(h)
    return h, owner, tag, dev.grid_fetch(h, n_fields, s.npts, dtype)


def _check_values(name, what, mesh, s, owner, fields, frame):
    """NaN exactly where the owner is -1; elsewhere within the bound of the host value.  Returns the largest error / bound."""
    pts, worst = s.points(), 0.0
    found = owner >= 0
    for q, u in enumerate(fields):
        want = s.sample(u, 1 if u.shape[1] == mesh.gdim + 1 else 2, owner, G.located(name, what)[1])
        assert np.array_equal(np.isnan(frame[q]), ~found), (name, what, q)
        bound = G.value_bound(mesh, pts, owner, u)
        ratio = np.abs(frame[q][found] - want[found]) / bound[found]
        worst = max(worst, float(ratio.max()))
    return worst


@pytest.mark.parametrize("name,p", [("2d", 1), ("2d", 2), ("3d", 1), ("3d", 2), ("emix", 1)])
def test_generic_position(hip_lib, name, p):
    """The table of the issue: 37x29 on make_mesh_2D(0) (825 of 1073 points inside), 23x19x17 on make_mesh_3D(0, n_axons=4) (5100 of
    7429) and on the EMIx submesh (3025 of 7429).  No point has a barycentric coordinate of magnitude below 1e-7 in any candidate
    cell (checked first, on the host), so owners must be exactly the host's."""
    mesh, sub, _ = G.mesh_tuple(name)
    s = G.spec(name, "generic")
    pi, ci, lam = G.candidates(name, "generic")
    print("%s: smallest |lambda| over %d candidate pairs %.2e" % (name, len(pi), np.abs(lam).min()))
    assert len(np.unique(pi)) >= G.SHAPES[name][1] and np.abs(lam).min() >= 1e-7
    h_owner = G.located(name, "generic")[0]
    assert (h_owner >= 0).sum() == G.SHAPES[name][1]
    pb = G.problem(name, p)
    fields = G.nodal_fields(pb)
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        _, owner, tag, frame = _frame(dev, s, len(fields))
        assert np.array_equal(owner, h_owner)
        tags = np.asarray(sub.array()).astype(np.int64)
        assert np.array_equal(tag, np.where(h_owner >= 0, tags[np.maximum(h_owner, 0)], -1))
        worst = _check_values(name, "generic", mesh, s, h_owner, fields, frame)
        print("%s P%d: largest error / bound %.2e" % (name, p, worst))
        assert worst < 1.0
    finally:
        dev.close()


@pytest.mark.parametrize("name,p", [("2d", 1), ("2d", 2), ("3d", 1), ("3d", 2)])
def test_points_on_facets_edges_and_vertices(hip_lib, monkeypatch, name, p):
    """A grid from xmin to xmax exactly (33x33, 17x9x9): 95 / 1265 points lie in several cells.  Accepted coordinates are >= -1e-14
    and rejected ones <= -1e-3 (asserted), nothing sits near the tolerance, so the lowest-index rule must hold exactly.  An affine
    nodal field comes back as a.p + b; a context built with KNP_NO_REORDER=1 gives the same owners and the same bits."""
    from knpemidg import _abi as A
    mesh, sub, _ = G.mesh_tuple(name)
    s = G.spec(name, "exact")
    pi, ci, lam = G.candidates(name, "exact")
    mn = lam.min(axis=1)
    ok = mn >= -1e-12
    print("%s: accepted min %.2e, rejected max %.2e" % (name, mn[ok].min(), mn[~ok].max()))
    assert mn[ok].min() >= -1e-14 and mn[~ok].max() <= -1e-3
    assert (np.bincount(pi[ok], minlength=s.npts) > 1).sum() == G.SHAPES[name][3]
    h_owner = G.located(name, "exact")[0]
    assert (h_owner >= 0).all()
    pb = G.problem(name, p)
    fields = G.nodal_fields(pb)
    # affine data at the nodes: vertices, then (P2) the edge midpoints in the local dof order
    x = mesh.coords[mesh.cells]
    if p == 2:
        nv = x.shape[1]
        x = np.concatenate([x, np.stack([0.5 * (x[:, a] + x[:, b]) for a in range(nv) for b in range(a + 1, nv)], axis=1)], axis=1)
    L = mesh.coords.max(axis=0) - mesh.coords.min(axis=0)
    a, b = np.array([0.7, -1.3, 2.1])[:mesh.gdim] / L, 0.4
    affine = x @ a + b
    pts = s.points()
    frames = []
    for reorder in (True, False):
        if not reorder:
            monkeypatch.setenv("KNP_NO_REORDER", "1")
        dev = device_for(pb)
        try:
            assert np.array_equal(dev.cell_order, np.arange(mesh.num_cells())) == (not reorder)
            push_state(dev, pb)
            _, owner, tag, frame = _frame(dev, s, len(fields))
            assert np.array_equal(owner, h_owner)
            dev.upload(A.F_PHI, affine)
            h2, _, _, aff = _frame(dev, s, 1)
            frames.append((owner, frame, aff))
        finally:
            dev.close()
    worst = _check_values(name, "exact", mesh, s, h_owner, fields, frames[0][1])
    err = np.abs(frames[0][2][0] - (pts @ a + b)) / G.value_bound(mesh, pts, h_owner, affine)
    print("%s P%d: largest error / bound %.2e (synthetic), %.2e (affine)" % (name, p, worst, err.max()))
    assert worst < 1.0 and err.max() < 1.0
    assert np.array_equal(frames[0][0], frames[1][0])
    assert frames[0][1].tobytes() == frames[1][1].tobytes() and frames[0][2].tobytes() == frames[1][2].tobytes()


def test_tags_slices_fp32_and_several_grids(hip_lib):
    """On the 3D mesh: tags=(1,) leaves only cells of that tag and gives the points on the membrane (32 of the 33x9x9 grid, 16 of
    which an extracellular cell owns without the filter) to the intracellular side; a slice equals the plane of its volume; an fp32
    frame is the fp64 frame rounded; two grids on one context do not disturb each other, and a third waiting frame is refused."""
    from knpemidg import _abi as A
    mesh, sub, _ = G.mesh_tuple("3d")
    tags = np.asarray(sub.array()).astype(np.int64)
    lo, hi = G.exact_bounds(mesh)
    pb = G.problem("3d", 1)
    nf = len(G.nodal_fields(pb))
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        # -- tag filter
        vol33, ics, ecs = (GridSpec(3, lo, hi, (33, 9, 9), tags=t) for t in (None, (1,), (0,)))
        want = ics.locate(mesh, tags)[0]
        h_all, o_all, _, f_all = _frame(dev, vol33, nf)
        h_ics, o_ics, t_ics, f_ics = _frame(dev, ics, nf)
        assert np.array_equal(o_ics, want) and np.array_equal(o_all, vol33.locate(mesh)[0])
        found = o_ics >= 0
        assert (tags[o_ics[found]] == 1).all() and (t_ics[found] == 1).all() and (t_ics[~found] == -1).all()
        on_membrane = found & (ecs.locate(mesh, tags)[0] >= 0)
        assert on_membrane.sum() == 32 and (tags[o_all[on_membrane]] == 0).sum() == 16
        assert np.isnan(f_ics[:, ~found]).all()
        same = found & (o_all == o_ics)
        assert np.array_equal(f_ics[:, same], f_all[:, same]) and not np.array_equal(f_ics[:, on_membrane], f_all[:, on_membrane])
        dev.grid_destroy(h_ics)
        dev.grid_destroy(h_all)
        # -- a slice is a plane of the volume that contains it
        vol = G.spec("3d", "exact")
        k = 4
        z = lo[2] + k * vol.h[2]
        plane = GridSpec(3, (lo[0], lo[1], z), (hi[0], hi[1], z), (17, 9, 1))
        h_vol, o_vol, t_vol, f_vol = _frame(dev, vol, nf)
        h_pl, o_pl, t_pl, f_pl = _frame(dev, plane, nf)
        assert np.array_equal(o_pl, o_vol.reshape(9, 9, 17)[k].ravel()) and np.array_equal(t_pl, t_vol.reshape(9, 9, 17)[k].ravel())
        assert f_pl.tobytes() == np.ascontiguousarray(f_vol.reshape(nf, 9, 9, 17)[:, k]).tobytes()
        # -- fp32 frames are the fp64 frames rounded (generic position: NaN outside the mesh included)
        gen = G.spec("3d", "generic")
        h64, _, _, f64 = _frame(dev, gen, nf)
        h32, _, _, f32 = _frame(dev, gen, nf, dtype=np.float32)
        assert f32.dtype == np.float32 and np.isnan(f32).any() and np.array_equal(f32, f64.astype(np.float32), equal_nan=True)
        # -- independent grids: four live now; interleaved sampling, each fetch returns its own grid's frame of the state it sampled
        dev.grid_sample(h_vol)
        dev.upload(A.F_PHI, 2.0 * pb.phi + 0.01)
        dev.grid_sample(h_pl)
        dev.grid_sample(h_vol)
        with pytest.raises(A.KnpError, match="-5"):
            dev.grid_sample(h_vol)                       # both pinned buffers of this grid wait
        second_pl = dev.grid_fetch(h_pl, nf, plane.npts)
        first_vol, second_vol = dev.grid_fetch(h_vol, nf, vol.npts), dev.grid_fetch(h_vol, nf, vol.npts)
        assert first_vol.tobytes() == f_vol.tobytes() and second_vol.tobytes() != f_vol.tobytes()
        assert np.array_equal(second_vol[1:], f_vol[1:])          # only phi changed
        assert second_pl.tobytes() == np.ascontiguousarray(second_vol.reshape(nf, 9, 9, 17)[:, k]).tobytes()
        with pytest.raises(A.KnpError, match="no frame waits"):
            dev.grid_fetch(h_vol, nf, vol.npts)
        dev.grid_destroy(h_vol)
        dev.grid_sample(h_pl)
        assert dev.grid_fetch(h_pl, nf, plane.npts).tobytes() == second_pl.tobytes()
        t = dev.grid_timing(h_pl)
        assert len(t) == 4 and all(np.isfinite(v) and v >= 0.0 for v in t) and t[0] > 0.0
    finally:
        dev.close()


def test_refusals_leave_the_context_as_it_was(hip_lib):
    """A bad shape, a non-finite bound, a spacing that is not positive, an unknown field id, too many tags and a ninth grid fail
    before anything is uploaded; the checkpoint layout (knp_state_describe) is the same with and without grids."""
    from knpemidg import _abi as A
    mesh = G.mesh_tuple("2d")[0]
    s = G.spec("2d", "generic")
    pb = G.problem("2d", 1)
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        table0, bytes0 = dev.state_describe()
        for what, kw in (("shape", dict(shape=(37, 0))), ("finite", dict(lo=(np.nan, 0.0))), ("finite", dict(h=(np.inf, 1.0))),
                         ("positive", dict(h=(0.0, 1.0))), ("field id", dict(fields=[0, 4])), ("field id", dict(fields=[-1])),
                         ("2\\^31", dict(shape=(65536, 32768))), ("tags", dict(tags=range(9))), ("tol", dict(tol=-1.0))):
            args = dict(lo=s.lo, h=s.h, shape=s.shape, fields=[0, 1, 2, 3])
            args.update(kw)
            with pytest.raises(A.KnpError, match=what):
                dev.grid_create(**args)
        handles = [dev.grid_create(s.lo, s.h, s.shape, [0]) for _ in range(8)]
        assert sorted(handles) == list(range(8))
        with pytest.raises(A.KnpError, match="at most 8"):
            dev.grid_create(s.lo, s.h, s.shape, [0])
        table1, bytes1 = dev.state_describe()
        assert bytes1 == bytes0 and table1.tobytes() == table0.tobytes()
        dev.grid_destroy(handles[3])
        assert dev.grid_create(s.lo, s.h, s.shape, [0, 3]) == 3          # the freed slot
        with pytest.raises(A.KnpError, match="no grid"):
            dev.grid_sample(11)
        dev.grid_sample(3)
        frame = dev.grid_fetch(3, 2, s.npts)
        owner = G.located("2d", "generic")[0]
        assert np.array_equal(np.isnan(frame[0]), owner < 0)
    finally:
        dev.close()


def _solver():
    from idealized_common import make_solver, solver_parameters
    sp = solver_parameters(3, 0, emi_dg_chebyshev=True)
    return make_solver(dim=3, resolution=0, n_axons=1, mesh_tuple=small_3d()), sp


def _grid_args(mesh):
    lo, hi = G.generic_bounds(mesh)
    return lo, hi, (13, 7, 5)


def test_frames_of_a_time_loop(hip_lib, tmp_path, monkeypatch):
    """10 steps of solve_system_active with every=5 write 3 frames (steps 0, 5, 10) of a volume and of a
    slice; each equals sampler.sample() taken by hand at those steps of a second run, /t and /step are right, the sidecar is there,
    and Solver.record_grid refuses what the host refuses."""
    from idealized_common import Constant
    from knpemidg import _abi as A
    from knpemidg.h5lite import H5File
    from knpemidg import setup_worker
    monkeypatch.setenv("KNP_NO_AMG", "1")
    # no hierarchy is built here, so no helper process may be started either: make_solver starts them ahead of time, they keep the
    # environment of that moment, and an idle one would serve a later test's solver with this test's settings
    monkeypatch.setenv("KNP_AMG_SERIAL_SETUP", "1")
    idle = len(setup_worker._IDLE)
    fields = ("phi", "K", "Na")
    S, sp = _solver()
    lo, hi, shape = _grid_args(S.mesh)
    mid = 0.5 * (lo[2] + hi[2])
    g = S.record_grid(lo, hi, shape, fields=fields, every=5)
    sl = S.record_grid((lo[0], lo[1], mid), (hi[0], hi[1], mid), (13, 7, 1), fields=("phi",), every=5, name="slice", dtype=np.float32)
    for bad in (dict(shape=(13, 7)), dict(lo=(0.0, np.nan, 0.0)), dict(fields=("phi", "Ca")), dict(name="grid")):
        args = dict(lo=lo, hi=hi, shape=shape, name="other")
        args.update(bad)
        with pytest.raises(A.KnpError):
            S.record_grid(**args)
    assert len(S.grids) == 2
    t = Constant(0.0)
    out = str(tmp_path / "run") + "/"
    S.solve_system_active(10 * 1e-4, t, sp, filename=out)
    assert sorted(os.listdir(out)) == ["grid.h5", "grid.xdmf", "slice.h5", "slice.xdmf"]
    cells, tags = g.cells.copy(), g.tags.copy()
    S.dev.close()
    # the second run, by hand
    S2, _ = _solver()
    g2 = S2.record_grid(lo, hi, shape, fields=fields)
    sl2 = S2.record_grid((lo[0], lo[1], mid), (hi[0], hi[1], mid), (13, 7, 1), fields=("phi",), name="slice", dtype=np.float32)
    S2._unpack_solver_params(sp)
    S2.save_fields = S2.save_solver_stats = False
    S2.splitting_scheme = True
    S2.setup_varform_emi(); S2.setup_varform_knp(); S2.setup_solver_emi(); S2.setup_solver_knp()
    t2 = Constant(0.0)
    want, want_sl, times = [g2.sample()], [sl2.sample()], [float(t2)]
    for k in range(10):
        S2.step_membrane_models(k)
        S2.solve_for_time_step(k, t2)
        if (k + 1) % 5 == 0:
            want.append(g2.sample())
            want_sl.append(sl2.sample())
            times.append(float(t2))
    S2.dev.close()
    h = H5File(out + "grid.h5")
    assert list(h.read("/step")) == [0, 5, 10] and list(h.read("/t")) == times and times[2] > times[1] > 0.0
    assert np.array_equal(h.read("/grid/cell"), cells) and np.array_equal(h.read("/grid/tag"), tags)
    assert cells.shape == (5, 7, 13) and (cells >= 0).any() and (cells < 0).any()
    assert np.array_equal(h.read("/grid/shape"), shape) and np.array_equal(h.read("/grid/lo"), lo)
    for n in range(3):
        for f in fields:
            a = h.read("/%s/vector_%d" % (f, n))
            assert a.shape == (5, 7, 13) and a.dtype == np.float64 and a.tobytes() == want[n][f].tobytes(), (n, f)
    assert not np.array_equal(want[0]["phi"], want[1]["phi"], equal_nan=True) and not np.array_equal(want[1]["K"], want[2]["K"], equal_nan=True)
    hs = H5File(out + "slice.h5")
    for n in range(3):
        a = hs.read("/phi/vector_%d" % n)
        assert a.shape == (1, 7, 13) and a.dtype == np.float32 and a.tobytes() == want_sl[n]["phi"].tobytes()
    assert "grid.h5:/K/vector_2" in open(out + "grid.xdmf").read()
    assert len(setup_worker._IDLE) == idle


def test_several_ranks_are_refused_without_hanging(hip_lib, tmp_path):
    """Two ranks on one GPU (shared-memory communicator): Solver.record_grid and the C entry point each raise the 'several ranks'
    error; no rank enters a collective, so nothing waits."""
    name = "/knp_%s" % uuid.uuid4().hex[:16]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "grid_rank_worker.py"), str(r), "2", name],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=120)
            logs.append(out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-2000:] for l in logs)
    assert all(l.count("several ranks") >= 2 for l in logs), logs
