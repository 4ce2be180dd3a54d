"""`Solver.record` on a partitioned solver, END TO END with several ranks on one GPU (the pattern of tests/test_gpu_multirank.py: one
process per rank, the shared-memory communicator in place of RCCL).  Every rank records what it owns; the partial rows are summed
over the ranks when the buffer is read; every rank must then hold the global rows.

Reference of the rows: the partitioned run's OWN fields.  Every worker dumps, per step, its owned cells' fields and its owned
membrane facets' phi_M / E / I_ch and gating variables; the parent reassembles them into global arrays and evaluates every channel
with the numpy formulation of tests/test_gpu_recorder.py (`expected_row`, `channel_errors`), bound 1e-11 of each channel's scale (the
same sums from the same doubles, in another order).  A one-GPU run is no reference for the potential: phi is determined up to a
constant that differs between partitions; only concentrations and phi_M are compared with it, at the bounds of the multirank test.
The partitions and the record arguments are those of tests/recorder_partition_cases.py; tests/test_recorder_partition_host.py
asserts that they reach every edge of the ownership rules."""
import os
import subprocess
import sys
import uuid
from types import SimpleNamespace

import numpy as np
import pytest

import knpemi_oracle as ko
import recorder_partition_cases as PC
from common import device_for, small_3d
from test_gpu_recorder import TOL, channel_errors, expected_row
from test_gpu_recorder_membrane import MAP_FIELDS, assert_map_equal, map_replica

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DT = 1.0e-4
IONS = ["K", "Cl", "Na"]


def _launch(outdir, case, capacity, mode="steps"):
    """The ranks of one run, at most three processes next to this one; every wait has a limit, stragglers are killed."""
    world = (PC.CASES.get(case) or PC.MORE_CASES[case])[0]
    os.makedirs(outdir)
    name = "/knp_%s" % uuid.uuid4().hex[:16]
    env = dict(os.environ, KNP_AMG_MAXCOARSE="300", KNP_AMG_DIST0="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "recorder_partition_worker.py"), str(r), str(world), name, outdir, case,
                               str(capacity), mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    logs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=240)
            logs.append(out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "%s capacity %d:\n%s" % (case, capacity, "\n".join(l[-2000:] for l in logs))
    return [dict(np.load(os.path.join(outdir, "rank%d.npz" % r))) for r in range(world)]


def _global_recorder(case):
    """The global tables, as every rank builds them."""
    from knpemidg import recorder as R
    mt, part, mtags, degree = PC.make_case(case)
    args, info = PC.record_args(mt, part, mtags)
    rec = R.Recorder(mt[0], mt[1].array(), mt[2].array(), degree, IONS, capacity=2, membrane_tags=mtags, membrane_states=PC.STATES,
                     membrane_map=dict(threshold=PC.MAP_THRESHOLD), **args)
    return SimpleNamespace(mt=mt, part=part, mtags=mtags, degree=degree, args=args, info=info, rec=rec)


def _host_rows(G, ranks):
    """(rows, scales, global phi_M per step, phi_M at arming) from the ranks' dumps: every channel of every step on the host."""
    from knpemidg import recorder as R
    from knpemidg.models import mm_hh, mm_hh_no_stim
    mesh, rec = G.mt[0], G.rec
    nc, nf, n_ions = mesh.num_cells(), mesh.num_facets(), len(IONS)
    seen_c, seen_f = np.zeros(nc, dtype=int), np.zeros(nf, dtype=int)
    for d in ranks:
        seen_c[d["cells"]] += 1
        seen_f[d["mem"]] += 1
    assert (seen_c == 1).all() and (seen_f[G.info["mem"]] == 1).all() and seen_f.sum() == len(G.info["mem"])
    odes = {1: mm_hh, 2: mm_hh_no_stim}
    models = [SimpleNamespace(ode=odes[t], tag=t) for t in G.mtags]
    chans = R.state_weights_global(mesh, rec.facet_tags, rec.set_facets, models, PC.STATES)
    wn = R.nodal_integration_weights(3, G.degree)
    sets = list(zip(rec.set_facets, rec.set_weights))
    rows, scales, phiM_steps = [], [], []
    v_arm = np.full(nf, np.nan)
    for d in ranks:
        v_arm[d["mem"]] = d["v_arm"]
    for k in range(PC.N_STEPS):
        nd = ranks[0]["fields"].shape[-1]
        fields = np.full((n_ions + 1, nc, nd), np.nan)
        memb = np.zeros((1 + 2 * n_ions, nf))
        st = np.full((len(PC.STATES), nf), np.nan)
        for d in ranks:
            fields[:, d["cells"]] = d["fields"][k]
            memb[:, d["mem"]] = d["membrane"][k]
            st[:, d["mem"]] = d["states"][k]
        row, sc = expected_row(list(fields), memb[0], memb[1:1 + n_ions], memb[1 + n_ions:], rec.point_cells, rec.point_w, sets, rec.region,
                               rec.n_regions, rec.vol, wn)
        srow, ssc = [], []
        for ch, (keep, w) in enumerate(chans):
            terms = w * st[ch % len(PC.STATES), rec.set_facets[ch // len(PC.STATES)][keep]]
            srow.append(terms.sum())
            ssc.append(np.abs(terms).sum())
        rows.append(np.concatenate([row, srow]))
        scales.append(np.concatenate([sc, ssc]))
        phiM_steps.append(memb[0].copy())
    return np.asarray(rows), np.asarray(scales), phiM_steps, v_arm


@pytest.fixture(scope="module")
def runs(hip_lib, tmp_path_factory):
    """Every partition once with capacity 2 (two reads on the way), slab3 once more with a buffer that holds every row.  The first
    failing run ends the fixture."""
    base = str(tmp_path_factory.mktemp("recpart"))
    out = {}
    for case, capacity in [(c, 2) for c in PC.CASES] + [("slab3", 64)]:
        ranks = _launch(os.path.join(base, "%s_cap%d" % (case, capacity)), case, capacity)
        G = _global_recorder(case)
        entry = SimpleNamespace(G=G, ranks=ranks)
        if capacity == 2:
            entry.host_rows, entry.host_scale, entry.phiM, entry.v_arm = _host_rows(G, ranks)
        out[(case, capacity)] = entry
    return out


@pytest.mark.parametrize("case", list(PC.CASES))
def test_rows_match_the_host_evaluation_of_the_runs_own_fields(runs, case):
    """Observed on the device: at most 4.4e-16 of a channel's scale over the four partitions (the test prints the figure per step)."""
    r = runs[(case, 2)]
    rows, rec = r.ranks[0]["rows"], r.G.rec
    n_ions = len(IONS)
    n_base = rec.n_points * (n_ions + 1) + rec.n_sets * (1 + 2 * n_ions) + rec.n_regions * (n_ions + 1)
    assert int(r.ranks[0]["n_base"]) == n_base and rows.shape == (PC.N_STEPS, n_base + rec.n_sets * len(PC.STATES))
    assert np.array_equal(r.ranks[0]["t"], r.ranks[0]["times"])
    for k in range(PC.N_STEPS):
        err = channel_errors(rows[k], r.host_rows[k], r.host_scale[k])
        print("%s step %d: worst channel error / scale %.2e (channel %d)" % (case, k, err.max(), int(err.argmax())))
        assert err.max() < TOL, (case, k, int(err.argmax()), err.max())
    # a channel whose terms are all exactly zero is exactly zero (chloride channel current of the Hodgkin-Huxley membranes), and the
    # inputs hold such channels
    zero = r.host_scale == 0.0
    assert zero.any() and (rows[zero] == 0.0).all()
    assert not np.array_equal(rows[0], rows[-1]) and np.isfinite(rows).all()


@pytest.mark.parametrize("case", list(PC.CASES))
def test_every_rank_holds_the_same_bits(runs, case):
    ranks = runs[(case, 2)].ranks
    for d in ranks[1:]:
        assert np.array_equal(d["rows"], ranks[0]["rows"]) and np.array_equal(d["t"], ranks[0]["t"])
        for name in MAP_FIELDS:
            assert np.array_equal(d["map_" + name], ranks[0]["map_" + name], equal_nan=True), name
        assert np.array_equal(d["map_facets"], ranks[0]["map_facets"])


def test_buffer_capacity_does_not_change_the_rows(runs):
    a, b = runs[("slab3", 2)].ranks, runs[("slab3", 64)].ranks
    for x, y in zip(a, b):
        assert np.array_equal(x["rows"], y["rows"]) and np.array_equal(x["t"], y["t"])
        for name in MAP_FIELDS:
            assert np.array_equal(x["map_" + name], y["map_" + name], equal_nan=True), name


def test_against_one_gpu(hip_lib, runs):
    """slab3 against a one-GPU `record` of the same arguments, where the null space of phi cancels: concentration probes and
    integrals at the multirank test's bound for c (1e-8), the phi_M set means at its bound for phi (1e-6, relative to max |phi_M|)."""
    from common_examples import make_solver, solver_parameters, Constant
    r = runs[("slab3", 2)]
    G = r.G
    S = make_solver(dim=3, resolution=0, n_axons=4, degree=1)
    try:
        rec1 = S.record(capacity=2, membrane_states=PC.STATES, membrane_map=dict(threshold=PC.MAP_THRESHOLD), **G.args)
        S._unpack_solver_params(solver_parameters(3, 0, emi_dg_chebyshev=True)._replace(rtol_emi=1e-10, rtol_knp=1e-12))     # as the workers
        S.save_fields = S.save_solver_stats = False
        S.splitting_scheme = True
        S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
        t = Constant(0.0)
        for k in range(PC.N_STEPS):
            S.step_membrane_models(k)
            if k == 0:
                rec1.arm(float(t))
            S.solve_for_time_step(k, t)
        one = SimpleNamespace(points=rec1.points, membrane=rec1.membrane, regions=rec1.regions, rows=rec1.rows.copy(), t=rec1.t.copy())
        assert np.array_equal(rec1.point_cells, G.rec.point_cells) and all(np.array_equal(a, b) for a, b in zip(rec1.set_facets, G.rec.set_facets))
    finally:
        S.dev.close()
    rec = G.rec
    rec._rows, rec._t = [r.ranks[0]["rows"]], [r.ranks[0]["t"]]           # the named views of the partitioned run's rows
    rec.n_base, rec._states_on_device = int(r.ranks[0]["n_base"]), True
    assert np.array_equal(one.t, rec.t) and one.rows.shape == rec.rows.shape
    for ion in IONS:
        for what, a, b in (("probe", rec.points[ion], one.points[ion]), ("integral", rec.regions[ion], one.regions[ion])):
            err = np.abs(a - b).max(axis=0) / np.abs(b).max(axis=0)
            print("%s %s: worst relative difference to one GPU %.2e" % (ion, what, err.max()))
            assert err.max() < 1e-8, (ion, what, err)
    a, b = rec.membrane["phi_M"], one.membrane["phi_M"]
    err = np.abs(a - b).max() / np.abs(b).max()
    print("phi_M set means: worst difference to one GPU / max |phi_M| %.2e" % err)
    assert err < 1e-6


@pytest.mark.parametrize("case", list(PC.CASES))
def test_map_matches_the_host_replay(runs, case):
    """The merged map against the crossing rule replayed on the dumped phi_M (bounds of tests/test_gpu_recorder_membrane.py: NaN
    pattern, counts, peaks and their times exact, interpolated times to 1e-12 dt)."""
    r = runs[(case, 2)]
    G, d0 = r.G, r.ranks[0]
    facets = G.rec.map_facets
    assert np.array_equal(d0["map_facets"], facets)
    times = list(d0["times"])
    ref = map_replica(r.v_arm[facets], 0.0, [(times[k], r.phiM[k][facets]) for k in range(PC.N_STEPS)], PC.MAP_THRESHOLD, PC.MAP_THRESHOLD)
    # conditions on the input: facets of at least two ranks crossed, at least one facet did not
    crossed = ref["n_activations"] > 0
    owners = G.part.owner[G.mt[0].facet_cells[facets, 0]]
    print("%s: %d of %d facets crossed, owners of those %s" % (case, int(crossed.sum()), len(facets), np.unique(owners[crossed])))
    assert len(np.unique(owners[crossed])) >= 2
    # ... where the mesh has unstimulated axons (tag 2); the one-axon mesh of rcb3 is all tag 1 and crosses everywhere
    assert (~crossed).any() == (len(G.mtags) > 1)
    got = {name: d0["map_" + name] for name in MAP_FIELDS}
    assert_map_equal(got, ref, DT, case)
    assert got["n_activations"].dtype == np.int32 and np.array_equal(got["n_activations"], ref["n_activations"])
    cv = [float(d["cv"]) for d in r.ranks]
    print("%s: conduction velocity between sets %s: %.6e m/s" % ((case, PC.CV_SETS, cv[0])))
    assert np.isfinite(cv[0]) and all(c == cv[0] for c in cv)


def test_rank_0_alone_writes_the_file(hip_lib, tmp_path):
    from knpemidg.h5lite import H5File
    outdir = os.path.join(str(tmp_path), "file")
    ranks = _launch(outdir, PC.FILE_CASE, 2, mode="file")
    found = [os.path.join(dp, f) for dp, _, fs in os.walk(outdir) for f in fs if f.endswith(".h5")]
    assert found == [os.path.join(outdir, "run_timeseries.h5")], found
    G = _global_recorder(PC.FILE_CASE)
    rec, d0 = G.rec, ranks[0]
    rec._rows, rec._t = [d0["rows"]], [d0["t"]]
    rec.n_base, rec._states_on_device = int(d0["n_base"]), True
    h = H5File(found[0])
    assert d0["t"].shape == (PC.N_STEPS,) and np.array_equal(h.read("timeseries/t"), d0["t"])
    for group, data in (("points", rec.points), ("membrane", rec.membrane), ("regions", rec.regions)):
        for name, a in data.items():
            got = h.read("timeseries/%s/%s" % (group, name))
            assert got.shape == a.shape and np.array_equal(got, a), (group, name)
    assert set(rec.membrane) >= set(PC.STATES) | {"phi_M"}
    assert np.array_equal(h.read("probes/cells"), rec.point_cells) and np.array_equal(h.read("membrane_sets/set_0/facets"), rec.set_facets[0])
    assert np.array_equal(h.read("membrane_map/facets"), rec.map_facets)
    for name in MAP_FIELDS[:4]:
        assert np.array_equal(h.read("membrane_map/" + name), d0["map_" + name], equal_nan=True), name
    assert np.array_equal(h.read("membrane_map/n_activations"), d0["map_n_activations"])
    assert np.array_equal(ranks[1]["rows"], d0["rows"])


# ---------------------------------------------------------------------------------------------------------------------
# refusals: one process, no communicator -- nothing here can leave a peer waiting
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_partition_mode_through_the_abi(hip_lib):
    """The unchanged entry points still refuse a -1 probe cell, an empty set and weights below 1; the partition-mode ones accept
    them, give exact zeros for what the rank does not own, and still refuse a facet that is no membrane facet and a region id >=
    n_regions before anything is uploaded."""
    from knpemidg import _abi as A
    from knpemidg import recorder as R
    from knpemidg.models import mm_hh
    from knpemidg.partition import Partition
    m, s, f = small_3d((8, 4, 4))
    loc = Partition(m, 2, method="slab").local(0)
    sub_l, surf_l = loc.localize(s, f, (1,))
    pb = ko.build_idealized(loc.mesh, sub_l.array(), surf_l.array(), membrane_tags=(1,))
    dev = device_for(pb, nc_owned=loc.nc_owned)
    try:
        lm, nc = loc.mesh, loc.mesh.num_cells()
        mem = R.membrane_facets(lm, surf_l.array(), [1])
        not_mem = int(np.nonzero(np.asarray(surf_l.array()) == 0)[0][0])
        w1 = np.full((2, 4), 0.25)
        region = np.zeros(nc, dtype=np.uint8)
        region[::2] = 1
        vol = R.cell_volumes(lm)
        inv = np.array([2.0e18, 0.0])
        n_states = len(mm_hh.init_state_values())
        h = dev.ode_create(mm_hh.MODEL_ID, mem, np.tile(np.linspace(0.1, 0.4, n_states), (len(mem), 1)),
                           np.tile(mm_hh.init_parameter_values(), (len(mem), 1)))
        no_rec = lambda: dev.lib.knp_rec_channels(dev.ctx) < 0
        # ---- the unchanged entry points
        with pytest.raises(A.KnpError, match="not an owned cell"):
            pc = np.array([0, -1], dtype=np.int32)
            sp = np.zeros(1, dtype=np.int64)
            dev._chk(dev.lib.knp_rec_create(dev.ctx, 4, 2, A._p(pc, A._i32p), A._p(w1, A._f64p), 0, A._p(sp, A._i64p), None, None, 0, None, None),
                     "knp_rec_create")
        assert no_rec()
        with pytest.raises(A.KnpError, match="is empty"):
            dev.rec_create(4, [], np.zeros((0, 4)), np.array([0, 1, 1]), mem[:1], np.array([1.0]), 0, None, None)
        assert no_rec()
        n_base = dev.rec_create(4, [], np.zeros((0, 4)), np.array([0, 2]), mem[:2], np.array([0.5, 0.5]), 0, None, None)
        with pytest.raises(A.KnpError, match="do not sum to 1"):
            dev.rec_add_states([0, 2], [h, h], [0, 1], [0, 0], [0.5, 0.25])
        with pytest.raises(A.KnpError, match="is empty"):
            dev.rec_add_states([0, 2, 2], [h, h], [0, 1], [0, 0], [0.5, 0.5])
        with pytest.raises(A.KnpError, match="other mode"):
            dev.rec_add_states([0, 2], [h, h], [0, 1], [0, 0], [0.5, 0.25], part=True)
        assert dev.lib.knp_rec_channels(dev.ctx) == n_base
        dev.rec_destroy()
        # ---- partition mode refuses what it must, before anything is uploaded
        good = dict(capacity=4, point_cell=[0, -1], point_w=w1, set_ptr=np.array([0, 2, 2]), set_facet=mem[:2], set_w=np.array([0.25, 0.25]),
                    n_regions=2, region=region, vol=vol, inv_rvol=inv)
        for change, msg in ((dict(set_facet=np.array([mem[0], not_mem])), "facet %d is not a membrane facet" % not_mem),
                            (dict(set_facet=np.array([mem[0], lm.num_facets()])), "not a membrane facet"),
                            (dict(region=np.where(np.arange(nc) == 3, 2, region).astype(np.uint8)), "region id 2"),
                            (dict(point_cell=[0, -2]), "not an owned cell"), (dict(point_cell=[0, loc.nc_owned]), "not an owned cell"),
                            (dict(inv_rvol=np.array([np.nan, 0.0])), "inv_rvol"), (dict(set_ptr=np.array([0, 2, 1]), set_facet=mem[:1], set_w=np.array([0.25])), "negative length")):
            with pytest.raises(A.KnpError, match=msg):
                dev.rec_create(**dict(good, **change))
            assert no_rec()
            with pytest.raises(A.KnpError, match="no recorder"):
                dev.rec_sample(0.0)
        # ---- and accepts the rest: a probe of another rank and an empty set are exact zeros, the explicit inv_rvol is used
        rng = np.random.default_rng(3)
        dev.upload(A.F_PHI, rng.uniform(-1, 1, size=(nc, 4)))
        dev.upload(A.F_PHI_M, rng.uniform(-1, 1, size=lm.num_facets()))
        n_base = dev.rec_create(**good)
        assert n_base == 2 * 4 + 2 * 7 + 2 * 4
        with pytest.raises(A.KnpError, match="sum to more than 1"):
            dev.rec_add_states([0, 2, 2], [h, h], [0, 1], [0, 0], [0.75, 0.5], part=True)
        with pytest.raises(A.KnpError, match="other mode"):
            dev.rec_add_map(mem[:2], 0.0, 0.0)
        with pytest.raises(A.KnpError, match="not a membrane facet"):
            dev.rec_add_map([not_mem], 0.0, 0.0, positions=[1], n_global=3)
        with pytest.raises(A.KnpError, match="outside the map or taken twice"):
            dev.rec_add_map(mem[:2], 0.0, 0.0, positions=[1, 1], n_global=3)
        with pytest.raises(A.KnpError, match="outside the map or taken twice"):
            dev.rec_add_map(mem[:2], 0.0, 0.0, positions=[1, 3], n_global=3)
        assert dev.rec_add_states([0, 2, 2], [h, h], [0, 1], [0, 0], [0.5, 0.25], part=True) == n_base + 2
        dev.rec_add_map(mem[:2], 0.0, 0.0, positions=[2, 0], n_global=3)
        dev.rec_map_arm(0.0)
        dev.rec_sample(1.0)
        t, rows = dev.rec_read()
        assert list(t) == [1.0] and rows.shape == (1, n_base + 2) and np.isfinite(rows).all()
        assert (rows[0, :4] != 0.0).any() and (rows[0, 4:8] == 0.0).all()                           # probe 1: cell -1
        assert rows[0, 8] != 0.0 and (rows[0, 8 + 7:8 + 14] == 0.0).all()                           # set 1: empty
        phi = dev.download(A.F_PHI).reshape(nc, 4)
        own = np.arange(nc) < loc.nc_owned
        for r in range(2):
            sel = own & (region == r)
            ref = (vol[sel] * phi[sel].mean(axis=1)).sum() * inv[r]
            assert rows[0, 22 + 4 * r + 3] == pytest.approx(ref, rel=1e-11, abs=0.0)
        assert rows[0, n_base] == pytest.approx(0.75 * 0.1, rel=1e-14) and rows[0, n_base + 1] == 0.0     # state channels: partial, empty
        act, rep, peak, tpk, n_up = dev.rec_map_read()
        phiM = dev.download(A.F_PHI_M)
        assert np.isnan(act[[0, 2]]).all() and act[1] == 0.0 and np.array_equal(peak, [phiM[mem[1]], 0.0, phiM[mem[0]]])
        assert n_up.dtype == np.int32 and (n_up == 0).all()
    finally:
        dev.close()
