"""Volume-field sampler on the mesh on the device (csrc/fieldmesh.hip) against the host statement of knpemidg/fieldmesh.py, which
tests/test_fieldmesh_host.py ties to an independent loop in extended precision.  The kernel makes the same IEEE operations in the same
order as FieldMeshSpec.sample_host, so every comparison is bit for bit: every case continuous and not, all cells and the ECS alone, fp64
and fp32 frames; a context without cell reordering; the guarded tail, a one-cell selection and four samplers side by side; refusals that
leave the context as it was; the frames a time loop writes, a resumed run's second part, and the several-ranks refusal."""
import gc
import os
import subprocess
import sys
import uuid
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import fieldmesh_cases as FC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples", "idealized_geometries"))
KNP_BLOCK = 256


@pytest.fixture(scope="module", autouse=True)
def _release_shared_references():
    """The meshes, problems, selections and references are computed once and shared by the tests of this module; released when it ends."""
    yield
    for cached in (FC.mesh_tuple, FC.spec, FC.problem, FC.brute):
        cached.cache_clear()
    gc.collect()


def _device_spec(dev, name, p, sel, cont, **kw):
    return FC.make_spec(name, p, sel, cont, cell_rank=dev.cell_rank, **kw)


def _check(dev, pb, s, names=None):
    """fp64 and fp32 frames of a spec against its host statement, bit for bit; returns the fp64 frame."""
    fields = FC.fields_of(pb)
    names = FC.field_names(pb) if names is None else names
    want = s.sample_host({q: fields[q] for q in names})
    h64, f64 = FC.device_frame(dev, pb, s, names)
    h32, f32 = FC.device_frame(dev, pb, s, names, dtype=np.float32)
    try:
        for q in names:
            assert f64[q].dtype == np.float64 and f64[q].shape == (s.n_nodes,)
            assert f64[q].tobytes() == want[q].tobytes(), (q, float(np.abs(f64[q] - want[q]).max()))
            assert f32[q].dtype == np.float32 and f32[q].tobytes() == want[q].astype(np.float32).tobytes(), q
        ts = dev.fieldmesh_timing(h64)
        assert len(ts) == 2 and all(np.isfinite(v) and v >= 0.0 for v in ts) and ts[0] > 0.0
    finally:
        dev.fieldmesh_destroy(h64)
        dev.fieldmesh_destroy(h32)
    return f64


@pytest.mark.parametrize("name,p", FC.CASES)
def test_every_case_bit_for_bit(hip_lib, name, p):
    """All cells and the ECS alone, continuous and not: from 66 cells in 2D (fewer nodes than a block) to 155 280 nodal values in 3D P2
    (several hundred blocks and a tail).  The continuous output of all cells of the 2D mesh is refused (fieldmesh_cases)."""
    dev, pb = FC.device_case(name, p)
    try:
        assert not np.array_equal(dev.cell_order, np.arange(pb.mesh.num_cells()))
        for sel in FC.SELECTIONS:
            for cont in (True, False):
                if FC.refused(name, sel, cont):
                    with pytest.raises(ValueError, match="separates two selected cells"):
                        _device_spec(dev, name, p, sel, cont)
                    continue
                s = _device_spec(dev, name, p, sel, cont)
                f64 = _check(dev, pb, s)
                if cont:
                    assert np.diff(s.ptr).max() > 1
                    # the same numbers as the independent loop, through the host statement's tie to it
                    col, mean, scale, count = FC.brute(name, p, sel)
                    at = np.asarray([col[k] for k in FC.node_keys(s)])
                    for k, q in enumerate(FC.field_names(pb)):
                        assert (np.abs(f64[q].astype(np.longdouble) - mean[k][at]) <= FC.BOUND * scale[k][at]).all(), q
                else:
                    u = FC.fields_of(pb)["phi"]
                    assert f64["phi"].tobytes() == np.ascontiguousarray(u[s.cell, s.dof]).tobytes()
    finally:
        dev.close()


@pytest.fixture(scope="module")
def no_reorder_frames(tmp_path_factory):
    """The frames of every case from contexts built with KNP_NO_REORDER=1, computed by one fresh child process."""
    out = str(tmp_path_factory.mktemp("fieldmesh") / "frames.npz")
    env = dict(os.environ, KNP_NO_REORDER="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "fieldmesh_frame_worker.py"), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return np.load(out)


@pytest.mark.parametrize("name,p", FC.CASES)
def test_no_reorder_gives_the_same_bits(hip_lib, no_reorder_frames, name, p):
    """The lists are ordered by the caller's cell ids, so the values do not depend on the device's cell order; the node numbering
    does, so the frames are matched by (entity, tag), resp. (cell, dof)."""
    sel = "ecs" if name == "2d" else "all"
    dev, pb = FC.device_case(name, p)
    try:
        assert not np.array_equal(dev.cell_order, np.arange(pb.mesh.num_cells()))
        mine = {}
        for cont in (True, False):
            s = _device_spec(dev, name, p, sel, cont)
            h, frame = FC.device_frame(dev, pb, s)
            dev.fieldmesh_destroy(h)
            mine[cont] = (s, frame)
    finally:
        dev.close()
    assert int(no_reorder_frames["%s_p%d_identity" % (name, p)]) == 1
    for cont, (s, frame) in mine.items():
        key = "%s_p%d_%d" % (name, p, cont)
        other = no_reorder_frames[key]                                  # [n_fields, n_nodes]
        a = no_reorder_frames[key + "_a"]                               # entity / cell of the other context's nodes
        b = no_reorder_frames[key + "_b"]                               # tag / dof
        mine_a, mine_b = (s.node_entity, s.node_tag) if cont else (s.cell, s.dof)
        big = int(max(a.max(), mine_a.max())) + 1
        theirs = b.astype(np.int64) * big + a
        by = np.argsort(theirs)
        at = by[np.searchsorted(theirs[by], mine_b * big + mine_a)]
        assert np.array_equal(np.sort(at), np.arange(s.n_nodes)) and not np.array_equal(at, np.arange(s.n_nodes))
        for k, q in enumerate(FC.field_names(pb)):
            assert frame[q].tobytes() == np.ascontiguousarray(other[k][at]).tobytes(), (cont, q)


def test_guarded_tail_one_cell_and_four_samplers(hip_lib):
    from knpemidg import _abi as A
    dev, pb = FC.device_case("3d", 1)
    try:
        # 4044 and 3216 nodes: 15 and 12 full blocks and a tail (the DG outputs of this mesh are whole blocks: test_every_case_bit_for_bit)
        specs = [_device_spec(dev, "3d", 1, "all", True), _device_spec(dev, "3d", 1, "ecs", True),
                 _device_spec(dev, "3d", 1, "all", True, cell_tags=FC.one_cell_tags("3d", 4321), tags=(7,)),
                 _device_spec(dev, "3d", 1, "all", False, cell_tags=FC.one_cell_tags("3d", 17), tags=(7,))]
        assert all(s.n_nodes % KNP_BLOCK != 0 for s in specs) and specs[0].n_nodes > KNP_BLOCK
        assert specs[2].n_sel == specs[3].n_sel == 1 and specs[2].n_nodes == specs[3].n_nodes == 4
        one = _check(dev, pb, specs[2])
        assert one["phi"].tobytes() == FC.fields_of(pb)["phi"][4321].tobytes()       # lists of length one: the cell's own values
        _check(dev, pb, specs[3], names=["c_K"])
        fields = FC.fields_of(pb)
        names = [FC.field_names(pb), ["phi"], ["c_Na", "phi"], FC.field_names(pb)[::-1]]
        made = [FC.device_frame(dev, pb, s, q, dtype=np.float32 if i == 1 else np.float64)[0] for i, (s, q) in enumerate(zip(specs, names))]
        assert sorted(made) == [0, 1, 2, 3]
        with pytest.raises(A.KnpError, match=r"\(-1\).*at most 4"):
            FC.device_frame(dev, pb, specs[0])
        dev.upload(A.F_PHI, 2.0 * pb.phi)                                             # the four sample the state as it is NOW
        for h in made:
            dev.fieldmesh_sample(h)
        for i, (h, s, q) in enumerate(zip(made, specs, names)):
            dtype = np.float32 if i == 1 else np.float64
            got = dev.fieldmesh_fetch(h, len(q), s.n_nodes, dtype)
            want = s.sample_host({k: (2.0 * fields[k] if k == "phi" else fields[k]) for k in q}, dtype=dtype)
            for row, k in zip(got, q):
                assert row.tobytes() == want[k].tobytes(), (i, k)
        dev.fieldmesh_destroy(made[1])
        assert FC.device_frame(dev, pb, specs[1], ["phi"])[0] == 1                    # the freed slot
    finally:
        dev.close()


def test_refusals_leave_the_context_as_it_was(hip_lib):
    from knpemidg import _abi as A
    dev, pb = FC.device_case("3d", 2)
    try:
        s = _device_spec(dev, "3d", 2, "ecs", True)
        nc, nd = pb.mesh.num_cells(), 10
        table0, bytes0 = dev.state_describe()
        phi = [(A.FM_PHI, -1), (A.FM_C, 2)]
        h0 = dev.fieldmesh_create(s.ptr, s.cell, s.dof, phi)
        assert h0 == 0
        dev.fieldmesh_sample(h0)
        before = dev.fieldmesh_fetch(h0, 2, s.n_nodes)
        ptr, cell, dof = s.ptr[:6].copy(), s.cell[:s.ptr[5]].copy(), s.dof[:s.ptr[5]].copy()
        assert len(cell) >= 6
        good = (ptr, cell, dof)

        def refused(msg, ptr=ptr, cell=cell, dof=dof, fields=phi, code=-1):
            with pytest.raises(A.KnpError, match=r"\(%d\).*%s" % (code, msg)):
                dev.fieldmesh_create(ptr, cell, dof, fields)
            h = dev.fieldmesh_create(*good, phi)                          # the context still takes a valid create
            assert h == 1
            dev.fieldmesh_destroy(h)

        bad = ptr.copy(); bad[3] = bad[2] - 1
        refused("strictly increasing.*node 2", ptr=bad)                   # non-monotone
        bad = ptr.copy(); bad[3] = bad[2]
        refused("list of node 2 is empty", ptr=bad)
        bad = ptr.copy(); bad[0] = 1
        refused("start at 0", ptr=bad)
        bad = cell.copy(); bad[4] = nc
        refused("cell %d .entry 4. outside" % nc, cell=bad)
        bad = cell.copy(); bad[1] = -1
        refused("cell -1 .entry 1. outside", cell=bad)
        bad = dof.copy(); bad[2] = nd
        refused("dof %d .entry 2. outside" % nd, dof=bad)
        bad = dof.copy(); bad[0] = -1
        refused("dof -1 .entry 0. outside", dof=bad)
        refused("ion 3 outside", fields=[(A.FM_C, 3)])
        refused("ion -1 outside", fields=[(A.FM_PHI, 0), (A.FM_C, -1)])
        refused("unknown kind 2", fields=[(2, 0)])
        refused("field planes", fields=[])
        refused("field planes", fields=[(A.FM_PHI, -1)] * 10)
        table1, bytes1 = dev.state_describe()
        assert bytes1 == bytes0 and table1.tobytes() == table0.tobytes()             # no checkpoint block, before or after
        dev.fieldmesh_sample(h0)
        assert dev.fieldmesh_fetch(h0, 2, s.n_nodes).tobytes() == before.tobytes()   # the existing sampler's next frame is unchanged
        with pytest.raises(A.KnpError, match="no field-mesh sampler"):
            dev.fieldmesh_sample(1)
        with pytest.raises(A.KnpError, match="no frame waits"):
            dev.fieldmesh_fetch(h0, 2, s.n_nodes)
        dev.fieldmesh_sample(h0)
        dev.upload(A.F_PHI, 2.0 * pb.phi)
        dev.fieldmesh_sample(h0)
        with pytest.raises(A.KnpError, match=r"\(-5\)"):
            dev.fieldmesh_sample(h0)                                      # both pinned buffers of this sampler wait
        with pytest.raises(A.KnpError, match=r"\(-1\).*must hold"):
            dev.fieldmesh_fetch(h0, 1, s.n_nodes)                         # the wrong byte count
        first, second = dev.fieldmesh_fetch(h0, 2, s.n_nodes), dev.fieldmesh_fetch(h0, 2, s.n_nodes)
        fields = FC.fields_of(pb)
        assert first.tobytes() == before.tobytes()
        assert second[0].tobytes() == s.sample_host({"phi": 2.0 * fields["phi"]})["phi"].tobytes() and second[1].tobytes() == before[1].tobytes()
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------- Solver level
FIELDS = ("phi", "c_K", "c_Na")            # Na is the eliminated ion of the idealized set-up
DT = 1.0e-4


def _solver():
    from idealized_common import make_solver, solver_parameters
    return make_solver(dim=2, resolution=0, mesh_tuple=FC.mesh_tuple("2d")), solver_parameters(2, 0)


def _attach(S):
    """every=1: the exact DG values of all cells, fp64; every=2: the continuous ECS, fp32 (the default).  (The continuous output of
    all cells of this mesh is refused: fieldmesh_cases.)"""
    return {"fields": S.record_fields(fields=FIELDS, continuous=False, every=1, dtype=np.float64),
            "ecs": S.record_fields(fields=FIELDS, tags=FC.ECS, every=2, name="ecs")}


def _nodal(S):
    ions = [ion['name'] for ion in S.ion_list]
    c = S.c.array().reshape(len(ions) - 1, S.mesh.num_cells(), -1)
    out = {"phi": S.phi.array().reshape(S.mesh.num_cells(), -1)}
    for k, ion in enumerate(ions[:-1]):
        out["c_" + ion] = c[k]
    out["c_" + ions[-1]] = S.ion_list[-1]['c'].array().reshape(S.mesh.num_cells(), -1)
    return {q: np.array(out[q]) for q in FIELDS}


def _check_sidecar(path, h, spec, n_frames, precision):
    root = ET.parse(os.path.splitext(path)[0] + ".xdmf").getroot()
    grids = root.find("Domain/Grid").findall("Grid")
    assert len(grids) == n_frames and [float(g.find("Time").get("Value")) for g in grids] == list(h.read("/t"))
    for k, g in enumerate(grids):
        assert g.find("Topology").get("TopologyType") == "Triangle" and int(g.find("Topology").get("NumberOfElements")) == spec.n_sel
        names = [a.get("Name") for a in g.findall("Attribute")]
        assert names == ["tag"] + list(FIELDS)
        for item in g.iter("DataItem"):
            fname, dset = item.text.strip().split(":/")
            a = h.read("/" + dset)
            assert fname == os.path.basename(path) and tuple(int(x) for x in item.get("Dimensions").split()) == a.shape
            assert int(item.get("Precision")) == a.dtype.itemsize
        assert g.findall("Attribute")[1].find("DataItem").text.strip().endswith("/phi/vector_%d" % k)
        assert int(g.findall("Attribute")[1].find("DataItem").get("Precision")) == precision


def test_frames_of_a_time_loop(hip_lib, tmp_path, monkeypatch):
    """Three steps on the 2D r = 0 solver: every=1 writes the frames of steps 0 .. 3, every=2 those of steps 0 and 2; each is the host
    statement of the fields a twin run that steps by hand holds at that step; phi and c after the run are the bits of a run without
    a sampler; a resumed run writes the second part."""
    from idealized_common import Constant
    from knpemidg import _abi as A
    from knpemidg import setup_worker
    from knpemidg.h5lite import H5File
    monkeypatch.setenv("KNP_NO_AMG", "1")
    monkeypatch.setenv("KNP_AMG_SERIAL_SETUP", "1")     # no hierarchy is built: no helper process may be started either (test_gpu_grid.py)
    idle = len(setup_worker._IDLE)
    S, sp = _solver()
    made = _attach(S)
    with pytest.raises(ValueError, match="separates two selected cells"):
        S.record_fields(name="smeared")
    with pytest.raises(ValueError, match="c_Ca"):
        S.record_fields(fields=("c_Ca",), name="other")
    with pytest.raises(ValueError, match="tag 9"):
        S.record_fields(tags=(9,), name="other")
    with pytest.raises(A.KnpError, match="exists already"):
        S.record_fields(tags=FC.ECS)
    assert len(S.fieldmeshes) == 2
    out = str(tmp_path / "with") + "/"
    S.solve_system_active(3 * DT, Constant(0.0), sp, filename=out, checkpoint_every=2)
    assert sorted(os.listdir(out)) == ["checkpoint.h5", "ecs.h5", "ecs.xdmf", "fields.h5", "fields.xdmf"]
    specs = {k: m.spec for k, m in made.items()}
    assert np.array_equal(made["ecs"].node_tag, np.zeros(specs["ecs"].n_nodes)) and made["fields"].connectivity.shape == (248, 3)
    phi, c = S.phi.array().copy(), S.c.array().copy()
    last = made["fields"].sample()
    assert set(last) == set(FIELDS) and made["fields"].timing()["sample_ms"] > 0.0
    S.dev.close()
    # the twin, by hand
    S2, _ = _solver()
    S2._unpack_solver_params(sp)
    S2.save_fields = S2.save_solver_stats = False
    S2.splitting_scheme = True
    S2.setup_varform_emi(); S2.setup_varform_knp(); S2.setup_solver_emi(); S2.setup_solver_knp()
    t2 = Constant(0.0)
    states, times = [_nodal(S2)], [float(t2)]
    for k in range(3):
        S2.step_membrane_models(k)
        S2.solve_for_time_step(k, t2)
        states.append(_nodal(S2))
        times.append(float(t2))
    assert S2.fieldmeshes is None
    assert S2.phi.array().tobytes() == phi.tobytes() and S2.c.array().tobytes() == c.tobytes()        # the samplers changed nothing
    S2.dev.close()
    for name, steps, dtype in (("fields", [0, 1, 2, 3], np.float64), ("ecs", [0, 2], np.float32)):
        h = H5File(out + name + ".h5")
        s = specs[name]
        assert list(h.read("/step")) == steps and list(h.read("/t")) == [times[k] for k in steps] and "step_offset" not in h.datasets
        assert np.array_equal(h.read("/mesh/node_entity"), s.node_entity) and np.array_equal(h.read("/mesh/connectivity"), s.connectivity)
        for n, k in enumerate(steps):
            want = s.sample_host(states[k], dtype=dtype)
            for q in FIELDS:
                a = h.read("/%s/vector_%d" % (q, n))
                assert a.dtype == dtype and a.tobytes() == want[q].tobytes(), (name, k, q)
        _check_sidecar(out + name + ".h5", h, s, len(steps), np.dtype(dtype).itemsize)
    assert all(last[q].tobytes() == specs["fields"].sample_host(states[3])[q].tobytes() for q in FIELDS)
    assert not np.array_equal(states[0]["phi"], states[1]["phi"]) and not np.array_equal(states[2]["c_K"], states[3]["c_K"])
    # the second part of a resumed run: from the checkpoint of step 2 to step 3
    S3, _ = _solver()
    made3 = _attach(S3)
    out3 = str(tmp_path / "resumed") + "/"
    S3.solve_system_active(3 * DT, Constant(0.0), sp, filename=out3, resume=out + "checkpoint.h5")
    S3.dev.close()
    assert sorted(os.listdir(out3)) == ["ecs_from2.h5", "ecs_from2.xdmf", "fields_from2.h5", "fields_from2.xdmf"]
    h3 = H5File(out3 + "fields_from2.h5")
    assert list(h3.read("/step_offset")) == [2] and list(h3.read("/step")) == [2, 3] and list(h3.read("/t")) == times[2:]
    for n, k in enumerate((2, 3)):
        want = made3["fields"].spec.sample_host(states[k])
        assert all(h3.read("/%s/vector_%d" % (q, n)).tobytes() == want[q].tobytes() for q in FIELDS), k
    assert list(H5File(out3 + "ecs_from2.h5").read("/step")) == [2]
    assert len(setup_worker._IDLE) == idle


def test_the_file_is_closed_when_the_loop_raises(hip_lib, tmp_path, monkeypatch):
    from idealized_common import Constant
    from knpemidg.h5lite import H5File
    monkeypatch.setenv("KNP_NO_AMG", "1")
    monkeypatch.setenv("KNP_AMG_SERIAL_SETUP", "1")
    S, sp = _solver()
    m = S.record_fields(fields=("phi",), continuous=False)
    calls = []
    step = S.solve_for_time_step

    def failing(k, t):
        if k == 2:
            raise RuntimeError("step 2 fails")
        calls.append(k)
        return step(k, t)

    S.solve_for_time_step = failing
    out = str(tmp_path) + "/"
    try:
        with pytest.raises(RuntimeError, match="step 2 fails"):
            S.solve_system_active(3 * DT, Constant(0.0), sp, filename=out)
        assert calls == [0, 1] and sorted(os.listdir(out)) == ["fields.h5", "fields.xdmf"]
        h = H5File(out + "fields.h5")
        assert list(h.read("/step")) == [0, 1, 2] and h.read("/phi/vector_2").dtype == np.float32
        assert m.sample()["phi"].tobytes() == h.read("/phi/vector_2").tobytes()       # no frame is left waiting
    finally:
        S.dev.close()


def test_a_sampler_made_after_the_device_context(hip_lib, monkeypatch):
    """record_fields before and after the device context exists give the same sampler."""
    monkeypatch.setenv("KNP_NO_AMG", "1")
    monkeypatch.setenv("KNP_AMG_SERIAL_SETUP", "1")
    S, sp = _solver()
    try:
        early = S.record_fields(tags=FC.ECS, name="early", dtype=np.float64)
        if S.dev is None:
            assert not early.attached
            S._ensure_device()
        late = S.record_fields(tags=FC.ECS, name="late", dtype=np.float64)
        assert early.attached and late.attached and np.array_equal(early.node_entity, late.node_entity)
        a, b = early.sample(), late.sample()
        want = early.spec.sample_host({"phi": S.phi.array()})
        assert a["phi"].tobytes() == b["phi"].tobytes() == want["phi"].tobytes()
        for k in range(2):
            S.record_fields(name="more%d" % k, continuous=False)
        from knpemidg import _abi as A
        with pytest.raises(A.KnpError, match="at most 4"):
            S.record_fields(name="fifth", continuous=False)
    finally:
        S.dev.close()


def test_several_ranks_are_refused_without_hanging(hip_lib):
    """Two ranks on one GPU (shared-memory communicator): Solver.record_fields and the C entry point each raise the 'several ranks'
    error; no rank enters a collective, so nothing waits."""
    name = "/knp_%s" % uuid.uuid4().hex[:16]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "fieldmesh_rank_worker.py"), str(r), "2", name],
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
