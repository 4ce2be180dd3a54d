"""Membrane-surface sampler on the device (csrc/surface.hip) against the host statement of knpemidg/surface.py, which
tests/test_surface_host.py ties to an independent quadrature statement: facet planes and state planes bit for bit, traces within
8 eps sum |w_a u_a| (surface_cases.BOUND) of the host statement and of what pcws_constant_project's kernel (knp_facet_trace) writes
on the same context; then fp32 frames, a context without cell reordering, selections and the guarded tail, refusals, the checkpoint
layout, the frames a time loop writes and the several-ranks refusal."""
import gc
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import surface_cases as SC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples", "idealized_geometries"))


@pytest.fixture(scope="module", autouse=True)
def _release_shared_references():
    """The meshes, problems and selections are computed once and shared by the tests of this module; released when it ends."""
    yield
    for cached in (SC.mesh_tuple, SC.spec):
        cached.cache_clear()
    gc.collect()


def _host_frame(pb, s, names, states, models, tables, E):
    from knpemidg.surface import resolve_fields
    ids = resolve_fields(names, SC.ion_names(pb))
    phi_M, _, I = SC.facet_arrays(pb)
    nodal = SC.nodal_fields(pb)
    st = None
    if states:
        handle, row, col = s.state_tables(models, states)
        st = [(q, handle[k], row[k], col[k]) for k, q in enumerate(states)]
    return s.sample_host(list(zip(names, ids)), phi_M=phi_M, E=E, I_ch=I, phi=nodal[0], conc=nodal[1:], states=st, state_tables=tables)


def _same_bits(a, b):
    """equal bit for bit, NaN where and only where the other has NaN"""
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and a[~nan].tobytes() == b[~nan].tobytes()


def _traced(pb):
    """(plane base name, nodal field [nc, nd], (field, species) of knp_facet_trace) of phi and every concentration"""
    from knpemidg import _abi as A
    nodal = SC.nodal_fields(pb)
    ions = SC.ion_names(pb)
    out = [("phi", nodal[0], (A.F_PHI, 0))]
    for k, ion in enumerate(ions):
        out.append(("c_" + ion, nodal[1 + k], (A.F_C, k) if k < len(ions) - 1 else (A.F_C_ELIM, 0)))
    return out


@pytest.mark.parametrize("name,p", SC.CASES)
def test_every_plane(hip_lib, name, p):
    """Every field and the state planes n (only mm_hh has it) and V on every membrane facet: 62 facets in 2D (fewer than a wave),
    1472 and 3750 in 3D (several blocks and a tail)."""
    names, states = None, SC.state_names(name)
    dev, pb, s, models, tables, E = SC.device_case(name, p)
    try:
        names = SC.all_fields(pb)
        want = _host_frame(pb, s, names, states, models, tables, E)
        h64, f64 = SC.device_frame(dev, pb, s, models, names, states)
        h32, f32 = SC.device_frame(dev, pb, s, models, names, states, dtype=np.float32)
        assert s.n % 256 != 0 and f64.shape == (len(names) + len(states), s.n) and f64.dtype == np.float64
        got = dict(zip(names + states, f64))
        for q in names:
            if q.endswith("_e") or q.endswith("_i"):
                continue
            assert got[q].tobytes() == want[q].tobytes(), q          # phi_M, E_*, I_ch_*: the uploaded bits; I_ch_total: the host sum
        for q in states:
            assert _same_bits(got[q], want[q]), q
        on1 = np.isin(s.facets, models[0].facets)
        assert np.array_equal(np.isnan(got["n"]), ~on1) and (len(models) == 1 or (~on1).any())
        worst = [0.0, 0.0]
        for base, u, (field, species) in _traced(pb):
            for side, suffix in ((0, "_e"), (1, "_i")):
                scale = s.trace(u, side)[1]
                assert (scale > 0.0).all()
                project = dev.facet_trace(field, species, side)[s.facets]      # what pcws_constant_project(plus / minus(u, n_g)) holds
                for k, ref in enumerate((want[base + suffix], project)):
                    ratio = np.abs(got[base + suffix] - ref) / (SC.BOUND * scale)
                    worst[k] = max(worst[k], float(ratio.max()))
        print("%s P%d: %d facets, largest error / bound %.3f (host statement), %.3f (knp_facet_trace)" % (name, p, s.n, worst[0], worst[1]))
        assert worst[0] < 1.0 and worst[1] < 1.0
        assert f32.dtype == np.float32 and np.array_equal(f32, f64.astype(np.float32), equal_nan=True)
        ts = dev.surf_timing(h64)
        assert len(ts) == 2 and all(np.isfinite(v) and v >= 0.0 for v in ts) and ts[0] > 0.0
    finally:
        dev.close()


@pytest.fixture(scope="module")
def no_reorder_frames(tmp_path_factory):
    """The frames of every case from contexts built with KNP_NO_REORDER=1, computed by one fresh child process."""
    out = str(tmp_path_factory.mktemp("surface") / "frames.npz")
    env = dict(os.environ, KNP_NO_REORDER="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "surface_frame_worker.py"), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return np.load(out)


@pytest.mark.parametrize("name,p", SC.CASES)
def test_no_reorder_gives_the_same_bits(hip_lib, no_reorder_frames, name, p):
    dev, pb, s, models, tables, E = SC.device_case(name, p)
    try:
        assert not np.array_equal(dev.cell_order, np.arange(pb.mesh.num_cells()))
        _, frame = SC.device_frame(dev, pb, s, models, SC.all_fields(pb), SC.state_names(name))
    finally:
        dev.close()
    other = no_reorder_frames["%s_p%d" % (name, p)]
    assert int(no_reorder_frames["%s_p%d_identity" % (name, p)]) == 1
    assert other.shape == frame.shape and _same_bits(frame, other)


def test_selections_and_the_guarded_tail(hip_lib):
    """tags=(2,), one explicit facet and n - 1 facets on the 3D mesh: each frame is the matching columns of the frame of every facet,
    in ascending facet order."""
    dev, pb, s, models, tables, E = SC.device_case("3d", 1)
    try:
        names, states = SC.all_fields(pb), ["n", "V"]
        _, full = SC.device_frame(dev, pb, s, models, names, states)
        mesh, sub, surf = SC.mesh_tuple("3d")
        from knpemidg.surface import SurfaceSpec
        mk = lambda **kw: SurfaceSpec(mesh, surf, sub, (1, 2), degree=1, **kw)
        k = int(np.nonzero(s.tags == 1)[0][100])                        # a facet of the axon whose model has both states
        rest = list(s.facets[:k]) + list(s.facets[k + 1:])
        for sel, st in ((mk(tags=(2,)), ["V"]), (mk(facets=[int(s.facets[k])]), ["n", "V"]), (mk(facets=rest[::-1]), ["n", "V"])):
            assert (np.diff(sel.facets) > 0).all() and sel.n % 256 != 0
            h, frame = SC.device_frame(dev, pb, sel, models, names, st)
            cols = np.searchsorted(s.facets, sel.facets)
            rows = list(range(len(names))) + [len(names) + states.index(q) for q in st]
            assert _same_bits(frame, full[rows][:, cols])
            dev.surf_destroy(h)
        assert mk(tags=(2,)).n == 1104 and mk(facets=rest).n == s.n - 1
    finally:
        dev.close()


def test_refusals_leave_the_context_as_it_was(hip_lib):
    from knpemidg import _abi as A
    dev, pb, s, models, tables, E = SC.device_case("3d", 1)
    try:
        mesh = pb.mesh
        table0, bytes0 = dev.state_describe()
        f = s.facets
        ok_fields = [(A.SF_PHI_M, -1), (A.SF_E, 1), (A.SF_TRACE_I, 2)]
        handle, row, col = s.state_tables(models, ["n"])
        interior = int(np.nonzero((mesh.facet_cells[:, 1] >= 0) & (pb.facet_tags == 0))[0][0])

        i1, i2 = (int(i) for i in np.nonzero(handle[0] >= 0)[0][[0, 3]])      # two facets whose model has the state

        def refused(code, msg, facets=None, fields=ok_fields, states=(handle, row, col)):
            with pytest.raises(A.KnpError, match=r"\(%d\).*%s" % (code, msg)):
                if facets is None:
                    dev.surf_create(f, fields, states=states)
                else:
                    dev.surf_create(facets, fields)
            h = dev.surf_create(f, ok_fields, states=(handle, row, col))        # the context still takes a valid create
            assert h == 0
            dev.surf_destroy(h)

        refused(-1, "facet %d .* not a membrane facet" % interior, facets=np.sort(np.append(f[:5], interior)))
        refused(-1, "not a membrane facet", facets=[-1])
        refused(-1, "not a membrane facet", facets=[mesh.num_facets()])
        refused(-1, "ascending", facets=f[::-1])
        refused(-1, "ascending", facets=np.append(f[:3], f[2]))
        refused(-1, "ion 3 outside", fields=[(A.SF_E, 3)])
        refused(-1, "ion -1 outside", fields=[(A.SF_I_CH, -1)])
        refused(-1, "ion -2 outside", fields=[(A.SF_TRACE_E, -2)])
        refused(-1, "ion 3 outside", fields=[(A.SF_TRACE_I, 3)])
        refused(-1, "unknown kind 6", fields=[(6, 0)])
        bad = row.copy(); bad[0, i1] = len(models[0].facets)
        refused(-1, "row %d outside" % len(models[0].facets), states=(handle, bad, col))
        bad = row.copy(); bad[0, i2] = -1
        refused(-1, "row -1 outside", states=(handle, bad, col))
        bad = col.copy(); bad[0, i2] = 4
        refused(-1, "column 4 outside", states=(handle, row, bad))
        bad = col.copy(); bad[0, i1] = -1
        refused(-1, "column -1 outside", states=(handle, row, bad))
        bad = handle.copy(); bad[0, i1] = 7
        refused(-1, "unknown ODE handle 7", states=(bad, row, col))
        bad = handle.copy(); bad[0, i2] = -2
        refused(-1, "unknown ODE handle -2", states=(bad, row, col))
        with pytest.raises(A.KnpError, match="planes"):
            dev.surf_create(f, [])
        hs = [dev.surf_create(f, ok_fields) for _ in range(4)]
        assert sorted(hs) == [0, 1, 2, 3]
        with pytest.raises(A.KnpError, match=r"\(-1\).*at most 4"):
            dev.surf_create(f, ok_fields)
        table1, bytes1 = dev.state_describe()
        assert bytes1 == bytes0 and table1.tobytes() == table0.tobytes()
        dev.surf_destroy(hs[2])
        assert dev.surf_create(f[:10], ok_fields) == 2                   # the freed slot
        with pytest.raises(A.KnpError, match="no surface sampler"):
            dev.surf_sample(3 + 4)
        with pytest.raises(A.KnpError, match="no frame waits"):
            dev.surf_fetch(0, 3, s.n)
        dev.surf_sample(0)
        dev.upload(A.F_PHI_M, 2.0 * pb.phi_M)
        dev.surf_sample(0)
        with pytest.raises(A.KnpError, match=r"\(-5\)"):
            dev.surf_sample(0)                                           # both pinned buffers of this sampler wait
        with pytest.raises(A.KnpError, match=r"\(-1\).*must hold"):
            dev.surf_fetch(0, 2, s.n)                                    # the wrong byte count
        with pytest.raises(A.KnpError, match=r"\(-1\).*must hold"):
            dev.surf_fetch(0, 3, s.n, np.float32)
        first, second = dev.surf_fetch(0, 3, s.n), dev.surf_fetch(0, 3, s.n)
        assert first[0].tobytes() == pb.phi_M[f].tobytes() and second[0].tobytes() == (2.0 * pb.phi_M)[f].tobytes()
        assert first[1:].tobytes() == second[1:].tobytes()
        dev.surf_sample(2)                                               # an independent sampler of 10 facets
        assert dev.surf_fetch(2, 3, 10).tobytes() == np.ascontiguousarray(second[:, :10]).tobytes()
    finally:
        dev.close()


def test_parameters_never_set_are_refused(hip_lib):
    from knpemidg import _abi as A
    pb = SC.problem("2d", 1)
    s = SC.spec("2d", 1)
    dev = A.Device(pb.mesh, pb.cell_tags, pb.facet_tags, pb.membrane_tags, len(pb.ions), degree=1)
    try:
        for kind in (A.SF_E, A.SF_I_CH, A.SF_I_CH_TOTAL):
            with pytest.raises(A.KnpError, match=r"\(-1\).*never set"):
                dev.surf_create(s.facets, [(kind, 0)])
        assert dev.surf_create(s.facets, [(A.SF_PHI_M, -1), (A.SF_TRACE_E, -1)]) == 0
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------- Solver level
FIELDS = ("phi_M", "E_K", "I_ch_Na", "c_K_e", "phi_i")


def _run(samplers, tmp_path, steps=3):
    """`steps` steps of solve_system_active on the 3D r = 0 mesh with the shipped models; samplers: {name: every}."""
    from idealized_common import Constant, make_solver, solver_parameters
    S = make_solver(dim=3, resolution=0, mesh_tuple=SC.mesh_tuple("3d"))
    sp = solver_parameters(3, 0, emi_dg_chebyshev=True)
    made = {k: S.record_membrane(every=every, fields=FIELDS, states=("n",), name=k) for k, every in samplers.items()}
    out = str(tmp_path) + "/"
    S.solve_system_active(steps * 1e-4, Constant(0.0), sp, filename=out)
    return S, made, out


def test_frames_of_a_time_loop(hip_lib, tmp_path, monkeypatch):
    """Three steps with every=1 write 4 frames, with every=2 the frames of steps 0 and 2; the last frame is what the solver's own
    fields give after the run; phi and the concentrations are the bytes of the same run without a sampler."""
    from knpemidg import _abi as A
    from knpemidg import setup_worker
    from knpemidg.h5lite import H5File
    from knpemidg.utils import minus, pcws_constant_project, plus
    monkeypatch.setenv("KNP_NO_AMG", "1")
    monkeypatch.setenv("KNP_AMG_SERIAL_SETUP", "1")     # no hierarchy is built: no helper process may be started either (test_gpu_grid.py)
    idle = len(setup_worker._IDLE)
    S, made, out = _run({"membrane": 1, "every2": 2}, tmp_path / "with")
    m = made["membrane"]
    assert sorted(os.listdir(out)) == ["every2.h5", "every2.xdmf", "membrane.h5", "membrane.xdmf"]
    h = H5File(out + "membrane.h5")
    t = h.read("/t")
    assert list(h.read("/step")) == [0, 1, 2, 3] and t[0] == 0.0 and (np.diff(t) > 0).all()
    f = h.read("/surface/facet")
    assert np.array_equal(f, m.facets) and len(f) == 1472 and h.read("/surface/connectivity").shape == (1472, 3)
    last = {q: h.read("/%s/vector_3" % q) for q in FIELDS + ("n",)}
    ions = [ion['name'] for ion in S.ion_list]
    kK, kNa = ions.index("K"), ions.index("Na")
    assert last["phi_M"].tobytes() == S.phi_M_prev_PDE.array()[f].tobytes()
    assert last["E_K"].tobytes() == S.ion_list[kK]['E'].array()[f].tobytes()
    I = S.dev.download(A.F_I_CH, 0, len(ions) * S.dev.nf).reshape(len(ions), -1)
    assert last["I_ch_Na"].tobytes() == I[kNa][f].tobytes()
    cK = S.c.split()[kK] if kK < len(ions) - 1 else S.ion_list[-1]['c']
    for q, proj, u in (("c_K_e", pcws_constant_project(plus(cK, S.n_g), S.Q).array()[f], cK.array()),
                       ("phi_i", pcws_constant_project(minus(S.phi, S.n_g), S.Q).array()[f], S.phi.array())):
        scale = m.spec.trace(u, 0 if q.endswith("_e") else 1)[1]
        assert (np.abs(last[q] - proj) <= SC.BOUND * scale).all(), q
    want_n = np.full(len(f), np.nan)
    for mm in S.mem_models:
        ode = mm['ode']
        pos = np.searchsorted(f, ode.facets)
        want_n[pos] = ode.states[:, ode.ode.state_indices("n")]
    assert _same_bits(last["n"], want_n) and not np.isnan(want_n).any()
    assert _same_bits(m.sample()["n"], want_n) and m.sample()["phi_M"].tobytes() == last["phi_M"].tobytes()
    first = h.read("/phi_M/vector_0")
    assert not np.array_equal(first, last["phi_M"])
    h2 = H5File(out + "every2.h5")
    assert list(h2.read("/step")) == [0, 2] and list(h2.read("/t")) == [t[0], t[2]]
    for q in FIELDS + ("n",):
        assert h2.read("/%s/vector_1" % q).tobytes() == h.read("/%s/vector_2" % q).tobytes()
        assert h2.read("/%s/vector_0" % q).tobytes() == h.read("/%s/vector_0" % q).tobytes()
    assert "membrane.h5:/c_K_e/vector_3" in open(out + "membrane.xdmf").read()
    phi, c = S.phi.array().copy(), S.c.array().copy()
    with pytest.raises(ValueError, match="E_Ca"):
        S.record_membrane(fields=("E_Ca",), name="other")
    with pytest.raises(ValueError, match="'q'"):
        S.record_membrane(states=("q",), name="other")
    with pytest.raises(A.KnpError, match="exists already"):
        S.record_membrane(name="membrane")
    assert len(S.surfaces_rec) == 2
    S.dev.close()
    S0, _, _ = _run({}, tmp_path / "without")
    assert S0.surfaces_rec is None
    assert S0.phi.array().tobytes() == phi.tobytes() and S0.c.array().tobytes() == c.tobytes()
    S0.dev.close()
    assert len(setup_worker._IDLE) == idle


def test_host_ode_refuses_states(hip_lib, monkeypatch):
    from idealized_common import make_solver
    from knpemidg import _abi as A
    from common import small_3d
    monkeypatch.setenv("KNP_HOST_ODE", "1")
    monkeypatch.setenv("KNP_NO_AMG", "1")
    monkeypatch.setenv("KNP_AMG_SERIAL_SETUP", "1")
    S = make_solver(dim=3, resolution=0, n_axons=1, mesh_tuple=small_3d())
    try:
        with pytest.raises(A.KnpError, match="KNP_HOST_ODE"):
            S.record_membrane(states=("n",))
        assert S.surfaces_rec is None
        assert set(S.record_membrane().sample()) == {"phi_M"}
    finally:
        S.dev.close()


def test_several_ranks_are_refused_without_hanging(hip_lib):
    """Two ranks on one GPU (shared-memory communicator): Solver.record_membrane and the C entry point each raise the 'several ranks'
    error; no rank enters a collective, so nothing waits."""
    name = "/knp_%s" % uuid.uuid4().hex[:16]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "surface_rank_worker.py"), str(r), "2", name],
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
