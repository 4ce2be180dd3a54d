"""The recorder's membrane additions on the device (csrc/record.hip: k_rec_states, k_rec_map) against numpy, through the C ABI and
through `Solver.record(membrane_states=..., membrane_map=...)`.

Map: the rules are comparisons and copies of identical doubles, so the NaN pattern, the counts, the peaks and their times agree
exactly; an interpolated time is one expression on identical inputs, where host and device differ at most by the contraction of a
multiply-add, a few ulp of t -- allowed: 1e-12 dt.

State channels: the device adds the same products in another order.  The bound comes from the reference computation alone: the
numpy mean in float64 (x64) and in np.longdouble (x_hp), allowed |device - x_hp| <= max(32 |x64 - x_hp|, 1e-15 sum|w x|).
The tests print the observed figures before they assert."""
import os
import sys

import numpy as np
import pytest

import knpemi_oracle as ko
from common import synthetic_state, device_for, push_state, small_3d

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "idealized_geometries"))

DT = 1.0e-4
MAP_FIELDS = ("activation_time", "repolarisation_time", "peak", "peak_time", "n_activations")


# ---------------------------------------------------------------------------------------------------------------------
# numpy replicas
# ---------------------------------------------------------------------------------------------------------------------
def map_replica(v_arm, t_arm, samples, thr, thr_r):
    """The rules of knp_rec_add_map (include/knpemi_hip.h) on the host.  samples = [(t, phi_M on the map's facets)]."""
    n = len(v_arm)
    prev, peak = v_arm.copy(), v_arm.copy()
    t_act, t_rep, t_peak, n_up = np.full(n, np.nan), np.full(n, np.nan), np.full(n, float(t_arm)), np.zeros(n, dtype=np.int32)
    t0 = float(t_arm)
    for t1, v1 in samples:
        v0 = prev
        with np.errstate(divide="ignore", invalid="ignore"):
            up = (v0 < thr) & (v1 >= thr)
            n_up[up] += 1
            first = up & np.isnan(t_act)
            t_act[first] = (t0 + (thr - v0) / (v1 - v0) * (t1 - t0))[first]
            down = ~np.isnan(t_act) & np.isnan(t_rep) & (v0 >= thr_r) & (v1 < thr_r)
            t_rep[down] = (t0 + (thr_r - v0) / (v1 - v0) * (t1 - t0))[down]
        higher = v1 > peak
        peak[higher] = v1[higher]
        t_peak[higher] = t1
        prev = v1.copy()
        t0 = float(t1)
    return dict(zip(MAP_FIELDS, (t_act, t_rep, peak, t_peak, n_up)))


def assert_map_equal(got, ref, dt, what):
    for name in ("activation_time", "repolarisation_time"):
        assert np.array_equal(np.isnan(got[name]), np.isnan(ref[name])), (what, name)
        ok = ~np.isnan(ref[name])
        err = np.abs(got[name][ok] - ref[name][ok]).max() / dt if ok.any() else 0.0
        print("%s: %s of %d facets, worst |device - host| = %.2e dt" % (what, name, int(ok.sum()), err))
        assert err <= 1e-12, (what, name, err)
    for name in ("peak", "peak_time", "n_activations"):
        assert np.array_equal(got[name], ref[name]), (what, name)


def state_reference(entries, tables):
    """Per channel (x64, x_hp, sum |w x|) from the entry lists and the host copies of the state tables {handle: [n, ns]}."""
    ptr, eh, er, ec, ew = entries
    out = []
    for s in range(len(ptr) - 1):
        sl = slice(ptr[s], ptr[s + 1])
        x = np.asarray([tables[int(h)][int(r), int(c)] for h, r, c in zip(eh[sl], er[sl], ec[sl])])
        out.append((float(np.dot(ew[sl], x)), float(np.sum(ew[sl].astype(np.longdouble) * x.astype(np.longdouble))), float(np.abs(ew[sl] * x).sum())))
    return np.asarray(out)


def state_errors(got, ref):
    """|device - x_hp| / bound per channel, bound = max(32 |x64 - x_hp|, 1e-15 sum |w x|)."""
    bound = np.maximum(32.0 * np.abs(ref[:, 0] - ref[:, 1]), 1e-15 * ref[:, 2])
    assert (bound > 0).all()
    return np.abs(np.asarray(got) - ref[:, 1]) / bound


# ---------------------------------------------------------------------------------------------------------------------
# the map kernel through the ABI
# ---------------------------------------------------------------------------------------------------------------------
REST, AMP, THR = -0.07, 0.1, -0.03
N_SAMPLES = 12


def pulse_fields(mesh, mem):
    """phi_M on the facets `mem` at samples 0 (arming) .. 12: two Gaussian pulses one behind the other that travel along x and stop
    short of the far end, so that facets near the start cross the threshold twice, those in the middle once and those at the far
    end never.  The last facet along x is put exactly on the threshold at samples 3 and 4 and back to rest at 5."""
    x = mesh.facet_midpoints()[mem, 0]
    xi = (x - x.min()) / (x.max() - x.min())
    g = lambda s: np.exp(-(s / 0.08) ** 2)
    out = [REST + AMP * (g(xi + 0.1 - 0.07 * k) + g(xi + 0.5 - 0.07 * k)) for k in range(N_SAMPLES + 1)]
    j = int(np.argmax(xi))
    for k in range(N_SAMPLES + 1):
        assert out[k][j] < REST + 1e-3                       # the pulses never get there
    out[3][j] = out[4][j] = THR
    return out, j


MAP_CASES = {"3D_own_repolarisation_level": ("3d", -0.05), "2D_two_vertex_facets": ("2d", THR)}


@pytest.mark.parametrize("case", list(MAP_CASES))
def test_map_kernel_against_numpy_through_the_abi(hip_lib, case):
    """A travelling double pulse pushed sample by sample into PHI_M; device map against the numpy replica, once with a buffer that
    holds every sample and once with capacity 5 (two reads on the way): the same bits.
    Device figures: not measured yet (the test prints them)."""
    from knpemidg import _abi as A
    from knpemidg import recorder as R
    from knpemidg.mesh import make_mesh_2D
    which, thr_r = MAP_CASES[case]
    m, s, f = make_mesh_2D(0) if which == "2d" else small_3d((7, 4, 4))
    pb = ko.build_idealized(m, s.array(), f.array(), p=1, membrane_tags=(1,))
    synthetic_state(pb)
    mem = R.membrane_facets(m, f.array(), [1])
    fields, j_thr = pulse_fields(m, mem)
    times = [k * DT for k in range(N_SAMPLES + 1)]
    ref = map_replica(fields[0], times[0], list(zip(times[1:], fields[1:])), THR, thr_r)
    # conditions on the input: every category of facet is there
    n_up, V = ref["n_activations"], np.asarray(fields)
    assert (n_up == 2).any() and (n_up == 1).any() and (n_up == 0).sum() >= 1
    assert (~np.isnan(ref["repolarisation_time"])).sum() >= 2          # up and down again
    assert ((V[1:] == THR) & (V[:-1] < THR)).any() and ((V[:-1] == THR) & (V[1:] == THR)).any() and ((V[:-1] == THR) & (V[1:] < THR)).any()
    assert n_up[j_thr] == 1 and ref["activation_time"][j_thr] == times[3]          # v1 == thr: crossed, at exactly that sample
    assert times[4] <= ref["repolarisation_time"][j_thr] < times[5] and (thr_r != THR or ref["repolarisation_time"][j_thr] == times[4])
    assert len(mem) < 256                                     # one partial workgroup; the solver-level and tag tests run several
    dev = device_for(pb)
    try:
        push_state(dev, pb)
        w = R.facet_areas(m, mem)
        results = []
        for capacity in (16, 5):
            phiM = np.zeros(m.num_facets())
            phiM[mem] = fields[0]
            dev.upload(A.F_PHI_M, phiM)
            dev.rec_create(capacity, [], np.zeros((0, pb.nd)), [0, len(mem)], mem, w / w.sum(), 0, None, None)
            dev.rec_add_map(mem, THR, thr_r)
            with pytest.raises(A.KnpError, match="not armed"):
                dev.rec_sample(0.0)
            dev.rec_map_arm(times[0])
            rows, waiting = [], 0
            for k in range(1, N_SAMPLES + 1):
                phiM[mem] = fields[k]
                dev.upload(A.F_PHI_M, phiM)
                if waiting == capacity:
                    rows.append(dev.rec_read()[1])
                    waiting = 0
                dev.rec_sample(times[k])
                waiting += 1
            rows.append(dev.rec_read()[1])
            rows = np.concatenate(rows)
            assert rows.shape == (N_SAMPLES, 7)
            got = dict(zip(MAP_FIELDS, dev.rec_map_read()))
            assert_map_equal(got, ref, DT, "%s capacity %d" % (case, capacity))
            results.append((rows, got))
        assert np.array_equal(results[0][0], results[1][0])
        for name in MAP_FIELDS:
            assert np.array_equal(results[0][1][name], results[1][1][name], equal_nan=True), name
        # a sample refused because the buffer is full leaves the map alone: prev is not advanced, nothing is counted
        dev.rec_create(1, [], np.zeros((0, pb.nd)), [0, len(mem)], mem, w / w.sum(), 0, None, None)
        dev.rec_add_map(mem, THR, thr_r)
        phiM[mem] = fields[0]
        dev.upload(A.F_PHI_M, phiM)
        dev.rec_map_arm(0.0)
        phiM[mem] = fields[2]
        dev.upload(A.F_PHI_M, phiM)
        dev.rec_sample(DT)
        before = dev.rec_map_read()
        phiM[mem] = fields[6]
        dev.upload(A.F_PHI_M, phiM)
        with pytest.raises(A.KnpError, match="-5"):
            dev.rec_sample(2 * DT)
        after = dev.rec_map_read()
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
        assert np.array_equal(before[2], np.maximum(fields[0], fields[2]))
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# state channels, tag selection and refusals on the two-tag mesh
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_tag(hip_lib):
    """The 4-axon r=0 mesh (368 membrane facets of tag 1, 1104 of tag 2) with a Hodgkin-Huxley table (4 states) on tag 1 and a
    glial one (1 state) on tag 2, both filled with seeded random numbers."""
    from types import SimpleNamespace
    from knpemidg import recorder as R
    from knpemidg.mesh import make_mesh_3D
    from knpemidg.models import mm_hh, mm_glial
    m, s, f = make_mesh_3D(0)
    pb = ko.build_idealized(m, s.array(), f.array(), p=1, membrane_tags=(1, 2))
    synthetic_state(pb)
    dev = device_for(pb)
    push_state(dev, pb)
    rng = np.random.default_rng(23)
    ft = np.asarray(f.array())
    models, tables = [], {}
    for tag, ode, mid in ((1, mm_hh, 1), (2, mm_glial, 4)):
        facets = R.membrane_facets(m, ft, [tag])
        st = rng.uniform(-1.0, 1.0, size=(len(facets), len(ode.init_state_values())))
        h = dev.ode_create(mid, facets, st, np.tile(ode.init_parameter_values(), (len(facets), 1)))
        models.append(SimpleNamespace(facets=facets, ode=ode, handle=h, tag=tag))
        tables[h] = st
    assert [len(x.facets) for x in models] == [368, 1104] and tables[models[0].handle].shape[1] == 4 and tables[models[1].handle].shape[1] == 1
    yield SimpleNamespace(mesh=m, sub=np.asarray(s.array()), surf=ft, pb=pb, dev=dev, models=models, tables=tables, rng=rng)
    dev.close()


def _two_tag_sets(T):
    """Sets and entry lists: all 368 HH facets (more than one pass of the 256-thread stride, with a tail), one single facet, a
    shuffled mix of both tags, and 300 glial facets -- n, m, h, V on the first three, V on the last."""
    from knpemidg import recorder as R
    hh, gl = T.models[0].facets, T.models[1].facets
    mix = np.concatenate([hh[::3], gl[::5]])
    mix = mix[np.random.default_rng(5).permutation(len(mix))]
    sets = [hh, hh[5:6], mix, gl[:300]]
    areas = [R.facet_areas(T.mesh, x) for x in sets]
    a = R.state_entries(sets[:3], areas[:3], T.models, ["n", "m", "h", "V"])
    b = R.state_entries(sets[3:], areas[3:], T.models, ["V"])
    entries = (np.concatenate([a[0], a[0][-1] + b[0][1:]]),) + tuple(np.concatenate([x, y]) for x, y in zip(a[1:], b[1:]))
    lengths = np.diff(entries[0])
    assert lengths.max() > 256 and lengths.max() % 256 != 0 and lengths.min() == 1 and len(lengths) == 13
    assert len(set(entries[1][entries[0][11]:entries[0][12]])) == 2            # V over the mix reads both handles
    return sets, areas, entries


def test_state_channels_against_numpy_through_the_abi(two_tag):
    """13 channels over two ODE handles with 4 and 1 states; two samples, the second after new tables were uploaded.
    Device error over bound: not measured yet (the test prints it per row)."""
    from knpemidg import _abi as A
    T, dev = two_tag, two_tag.dev
    sets, areas, entries = _two_tag_sets(T)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in sets])])
    create = (8, [], np.zeros((0, T.pb.nd)), ptr, np.concatenate(sets), np.concatenate([a / a.sum() for a in areas]), 0, None, None)
    n_base = dev.rec_create(*create)
    assert n_base == 4 * 7
    dev.rec_sample(0.5)
    plain = dev.rec_read()[1]
    dev.rec_create(*create)
    assert dev.rec_add_states(*entries) == n_base + 13
    dev.rec_sample(0.5)
    ref0 = state_reference(entries, T.tables)
    new = {h: T.rng.uniform(-1.0, 1.0, size=t.shape) for h, t in T.tables.items()}
    for x in T.models:
        dev.ode_table(x.handle, 0, new[x.handle].shape, upload=new[x.handle])
    dev.rec_sample(0.75)
    ref1 = state_reference(entries, new)
    for x in T.models:                                        # leave the fixture's tables as the other tests expect them
        dev.ode_table(x.handle, 0, new[x.handle].shape, upload=T.tables[x.handle])
    t, rows = dev.rec_read()
    assert list(t) == [0.5, 0.75] and rows.shape == (2, n_base + 13)
    for k, ref in enumerate((ref0, ref1)):
        err = state_errors(rows[k, n_base:], ref)
        print("state channels row %d: worst |device - x_hp| / bound %.2e (channel %d)" % (k, err.max(), int(err.argmax())))
        assert err.max() <= 1.0, (k, int(err.argmax()), err.max())
    assert not np.array_equal(rows[0, n_base:], rows[1, n_base:])
    # the single-entry channels are the table values themselves
    h0 = T.models[0]
    assert np.array_equal(rows[0, n_base + 4:n_base + 8], T.tables[h0.handle][5, [2, 0, 1, 3]])
    # the other channels of the same rows: bit for bit those of a recorder without state channels
    assert np.array_equal(rows[0, :n_base], plain[0]) and np.array_equal(rows[1, :n_base], plain[0])


def test_map_tags_select_a_subset(two_tag):
    """`tags=[2]` of the 4-axon mesh: 1104 facets (several workgroups, the last one partial); three samples against the replica."""
    from knpemidg import _abi as A
    from knpemidg import recorder as R
    T, dev = two_tag, two_tag.dev
    rec = R.Recorder(T.mesh, T.sub, T.surf, 1, ["K", "Cl", "Na"], regions=False, capacity=2, membrane_tags=[1, 2],
                     membrane_map=dict(threshold=-0.068, repolarisation=-0.072, tags=[2]))
    assert np.array_equal(rec.map_facets, T.models[1].facets) and len(rec.map_facets) % 256 != 0
    rec.attach(dev)
    rng = np.random.default_rng(31)
    mem = np.concatenate([x.facets for x in T.models])
    phiM = np.zeros(T.mesh.num_facets())
    fields = [-0.07 + 0.01 * rng.uniform(-1, 1, size=len(mem)) for _ in range(4)]
    phiM[mem] = fields[0]
    dev.upload(A.F_PHI_M, phiM)
    rec.arm(0.0)
    for k in range(1, 4):                                     # capacity 2: a flush before the third sample
        phiM[mem] = fields[k]
        dev.upload(A.F_PHI_M, phiM)
        rec.sample(k * DT)
    got = rec.membrane_map
    sel = slice(len(T.models[0].facets), None)
    ref = map_replica(fields[0][sel], 0.0, [(k * DT, fields[k][sel]) for k in range(1, 4)], -0.068, -0.072)
    assert np.array_equal(got["facets"], T.models[1].facets)
    assert (ref["n_activations"] > 0).any() and (ref["n_activations"] == 0).any() and (~np.isnan(ref["repolarisation_time"])).any()
    assert_map_equal(got, ref, DT, "tags=[2]")
    assert len(rec.t) == 3


def test_refusals_through_the_abi(two_tag):
    """Bad entries and a bad map facet: an error with a message, nothing uploaded -- the recorder keeps its channels and samples."""
    from knpemidg import _abi as A
    T, dev = two_tag, two_tag.dev
    hh, gl = T.models
    sets = [hh.facets[:4]]
    w = np.full(4, 0.25)
    n_base = dev.rec_create(4, [], np.zeros((0, T.pb.nd)), [0, 4], sets[0], w, 0, None, None)
    ok = ([0, 4], [hh.handle] * 4, [0, 1, 2, 3], [2] * 4, w)

    def refused(msg, ptr, eh, er, ec, ew):
        with pytest.raises(A.KnpError, match=msg):
            dev.rec_add_states(ptr, eh, er, ec, ew)
        assert dev.lib.knp_rec_channels(dev.ctx) == n_base
    refused("row 368 outside", ok[0], ok[1], [0, 1, 2, 368], ok[3], ok[4])
    refused("row -1 outside", ok[0], ok[1], [0, -1, 2, 3], ok[3], ok[4])
    refused("column 1 outside the handle's 1 states", ok[0], [hh.handle] * 3 + [gl.handle], ok[2], [2, 2, 2, 1], ok[4])
    refused("column 4 outside", ok[0], ok[1], ok[2], [2, 2, 4, 2], ok[4])
    refused("unknown ODE handle 7", ok[0], [hh.handle, 7, hh.handle, hh.handle], ok[2], ok[3], ok[4])
    refused("do not sum to 1", ok[0], ok[1], ok[2], ok[3], [0.25, 0.25, 0.25, 0.2])
    refused("do not sum to 1", ok[0], ok[1], ok[2], ok[3], [0.25, 0.25, np.nan, 0.25])
    refused("is empty", [0, 4, 4], ok[1], ok[2], ok[3], ok[4])
    not_mem = int(np.nonzero(T.surf == 0)[0][0])
    for bad, msg in (([int(hh.facets[0]), not_mem], "facet %d is not a membrane facet" % not_mem),
                     ([T.mesh.num_facets()], "not a membrane facet"), ([], "empty facet selection")):
        with pytest.raises(A.KnpError, match=msg):
            dev.rec_add_map(bad, 0.0, 0.0)
    with pytest.raises(A.KnpError, match="finite"):
        dev.rec_add_map(hh.facets, float("nan"), 0.0)
    dev.rec_sample(0.0)                                       # no map was stored: nothing to arm, the sample goes through
    t, rows = dev.rec_read()
    assert len(t) == 1 and rows.shape == (1, n_base)
    assert dev.rec_add_states(*ok) == n_base + 1              # the good list is accepted
    dev.rec_destroy()
    with pytest.raises(A.KnpError, match="no recorder"):      # before knp_rec_create
        dev.rec_add_states(*ok)
    with pytest.raises(A.KnpError, match="no recorder"):
        dev.rec_add_map(hh.facets, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# through the solver
# ---------------------------------------------------------------------------------------------------------------------
N_STEPS = 6
MAP_THRESHOLD = -0.04641253      # inside the range of phi_M after the sixth step, see test_solver_map_matches_the_host_replica
STATES = ("n", "m", "h")


def _run_3d(capacity, check=False):
    """Six steps of the 3D single-axon solver (the run of test_gpu_recorder.py); capacity None = no recorder, else one with the
    state channels n, m, h and a map.  Returns the final fields, the recorder's output and (check) what the host evaluates at
    every step from the downloaded state table and phi_M."""
    from idealized_common import make_solver, solver_parameters, Constant
    from knpemidg import recorder as R
    mt = small_3d((7, 4, 4))
    S = make_solver(dim=3, mesh_tuple=mt, n_axons=1)
    mesh, tags = mt[0], np.asarray(mt[1].array())
    rec = None
    if capacity is not None:
        mid = mesh.cell_midpoints()
        pts = [mid[np.nonzero(tags == 0)[0][10]], mid[np.nonzero(tags == 1)[0][10]], mesh.coords[mesh.cells[100, 2]]]
        box = (np.array([2.0e-6, 0.05e-6, 0.05e-6]), np.array([3.5e-6, 0.35e-6, 0.11e-6]))
        rec = S.record(points=pts, membrane_sets=[box, R.membrane_facets(mesh, mt[2].array(), [1])], regions=True, capacity=capacity,
                       membrane_states=STATES, membrane_map=dict(threshold=MAP_THRESHOLD))
    # the measured choice of the EMI smoother depends on timings: fixed here, so that two runs are the same computation
    S._unpack_solver_params(solver_parameters(3, 0, emi_dg_chebyshev=True))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    t = Constant(0.0)
    out = {"times": [], "state_ref": [], "phi_M": [], "v_arm": None}
    for k in range(N_STEPS):
        S.step_membrane_models(k)
        if k == 0 and rec is not None:
            rec.arm(float(t))                                 # by hand, where solve_system_active arms it
            out["v_arm"] = S.phi_M_prev_PDE.array()[rec.map_facets].copy()
        S.solve_for_time_step(k, t)
        out["times"].append(float(t))
        if check:
            model = S.mem_models[0]['ode']
            out["state_ref"].append(state_reference(rec.state_entry_lists, {model.handle: model.states}))
            out["phi_M"].append(S.phi_M_prev_PDE.array()[rec.map_facets].copy())
    out.update(phi=S.phi.array(), c=S.c.array())
    if rec is not None:
        n_ions = len(S.ion_list)
        out.update(t=rec.t.copy(), rows=rec.rows.copy(), membrane=rec.membrane, map=rec.membrane_map, n_base=rec.n_base,
                   set_sizes=[len(f) for f in rec.set_facets])
        assert rec.n_base == 3 * (n_ions + 1) + 2 * (1 + 2 * n_ions) + 2 * (n_ions + 1)
    S.dev.close()
    return out


@pytest.fixture(scope="module")
def runs(hip_lib):
    return {"cap4": _run_3d(4, check=True), "cap64": _run_3d(64), "none": _run_3d(None)}


def test_solver_state_channels_match_the_host_at_every_step(runs):
    """n, m, h over a box of facets and over the whole membrane, against the state table downloaded after every step (the row of
    step k holds the states after ODE step k).
    Device error over bound: not measured yet (the test prints it per step)."""
    r = runs["cap4"]
    assert r["rows"].shape == (N_STEPS, r["n_base"] + 2 * len(STATES)) and list(r["t"]) == r["times"]
    for k in range(N_STEPS):
        err = state_errors(r["rows"][k, r["n_base"]:], r["state_ref"][k])
        print("step %d: worst |device - x_hp| / bound %.2e" % (k, err.max()))
        assert err.max() <= 1.0, (k, int(err.argmax()), err.max())
    for q, name in enumerate(STATES):
        assert r["membrane"][name].shape == (N_STEPS, 2)
        assert np.array_equal(r["membrane"][name][:, 1], r["rows"][:, r["n_base"] + len(STATES) + q])
    n = r["membrane"]["n"]
    assert ((n > 0.0) & (n < 1.0)).all() and not np.array_equal(n[0], n[-1])          # gating variables, and they move
    assert r["set_sizes"][1] == 64 and 0 < r["set_sizes"][0] < 64


def test_solver_map_matches_the_host_replica(runs):
    """The map against the replica fed with phi_M_prev_PDE after every step.  Range of phi_M in this run, from an
    emulation on the host (the oracle's direct solves and the host ODE integrator; the device run's own figures are not entered
    yet, the test prints them): -0.068392 on all 64 facets at arming, then about 5 mV up per step -- -0.068392, -0.063108, -0.058431,
    -0.054237, -0.050340 -- to between -0.04641269 and -0.04641238 after step six.  The whole axon is stimulated, so the facets differ
    only in the seventh digit, and "some but not all activate" needs a threshold inside that last interval: MAP_THRESHOLD is its
    median.  The spread is of the size of the Krylov tolerance, so if the device run puts the interval elsewhere the assertion
    `0 < activated < 64` fails and the constant has to be taken from the printed range."""
    r = runs["cap4"]
    V = np.asarray([r["v_arm"]] + r["phi_M"])
    print("phi_M on the membrane: arming [%.6f, %.6f], then per step" % (V[0].min(), V[0].max()),
          ", ".join("[%.6f, %.6f]" % (v.min(), v.max()) for v in V[1:]))
    ref = map_replica(r["v_arm"], 0.0, list(zip(r["times"], r["phi_M"])), MAP_THRESHOLD, MAP_THRESHOLD)
    activated = int((~np.isnan(r["map"]["activation_time"])).sum())
    print("activated facets: %d of %d" % (activated, len(r["v_arm"])))
    assert_map_equal(r["map"], ref, DT, "solver")
    assert 0 < activated < len(r["v_arm"]) == 64
    assert np.array_equal(r["map"]["n_activations"] > 0, ~np.isnan(r["map"]["activation_time"]))


def test_solver_same_bits_again_and_with_another_capacity(runs):
    a, b = runs["cap4"], runs["cap64"]
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["t"], b["t"])
    for name in MAP_FIELDS:
        assert np.array_equal(a["map"][name], b["map"][name], equal_nan=True), name


def test_solver_fields_do_not_see_the_recorder(runs):
    a, n = runs["cap4"], runs["none"]
    assert np.array_equal(a["phi"], n["phi"]) and np.array_equal(a["c"], n["c"])


def test_host_ode_refuses_state_channels(hip_lib, monkeypatch):
    from idealized_common import make_solver
    from knpemidg import _abi as A
    monkeypatch.setenv("KNP_HOST_ODE", "1")
    mt = small_3d((7, 4, 4))
    S = make_solver(dim=3, mesh_tuple=mt, n_axons=1)
    try:
        mem = np.nonzero(np.asarray(mt[2].array()) == 1)[0]
        with pytest.raises(A.KnpError, match="KNP_HOST_ODE"):
            S.record(membrane_sets=[mem[:4]], regions=False, membrane_states=("n",))
        assert S.recorder is None
        S.record(membrane_sets=[mem[:4]], regions=False)       # without the state channels it is accepted as before
    finally:
        S.dev.close()


def test_timeseries_file_holds_the_new_datasets(hip_lib, tmp_path):
    from idealized_common import make_solver, solver_parameters, Constant
    from knpemidg.h5lite import H5File
    from knpemidg import recorder as R
    S = make_solver(dim=2, resolution=0)
    mem = R.membrane_facets(S.mesh, S.surfaces.array(), [1])
    rec = S.record(membrane_sets=[mem[:5], mem], regions=False, membrane_states=STATES, membrane_map=dict(threshold=-0.074, repolarisation=-0.0745))
    prefix = str(tmp_path) + os.sep + "run_"
    S.solve_system_active(3e-4, Constant(0.0), solver_parameters(2, 0), filename=prefix)
    h = H5File(prefix + "timeseries.h5")
    for name in STATES:
        got = h.read("timeseries/membrane/" + name)
        assert got.shape == (3, 2) and np.array_equal(got, rec.membrane[name]) and ((got > 0) & (got < 1)).all()
    m = rec.membrane_map
    assert np.array_equal(h.read("membrane_map/facets"), mem) and len(m["peak"]) == len(mem)
    for name in MAP_FIELDS[:4]:
        assert np.array_equal(h.read("membrane_map/" + name), m[name], equal_nan=True), name
    assert np.array_equal(h.read("membrane_map/n_activations"), m["n_activations"])
    assert list(h.read("membrane_map/threshold")) == [-0.074] and list(h.read("membrane_map/repolarisation")) == [-0.0745]
    assert np.isin(m["peak_time"], np.concatenate([[0.0], rec.t])).all()
    assert isinstance(rec.conduction_velocity(0, 1, method="set_mean"), float)        # a number or NaN, never an exception
    S.dev.close()
