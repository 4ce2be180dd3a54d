"""Several contexts alive in one process keep their solver state apart (csrc/solve.hip: Fields and the two PrecState records are
members of knp_ctx).

Solver A runs 4 steps alone.  Then B and C of the same configuration live together and take their steps interleaved (B0 B1 C0 B2 C1
B3 C2 C3), so that at every switch their solution histories, rebuild ages and spectral bounds differ.  Every step of B and of C must
leave what A's same step left: iteration counts, c, phi, phi_M and the whole state_save() snapshot (fields, both histories, both lagged
inverse arrays, every counter and bound).  The yardstick is a second lone run A': where A and A' do not agree bit for bit themselves,
four times their measured difference bounds B and C instead (as in tests/test_gpu_checkpoint.py).

The same holds for everything else a context owns (the library keeps no per-context state outside the
context): the unstructured-ring tables, the membrane-model sets, the recorder, the voxel grids, the checkpoint staging and the launch
caches of the persistent applies.  Two contexts of different kinds -- A on a jittered box (unstructured ring), B on a structured box
(ring with geometry classes) -- run one sequence through all of these, first interleaved on one thread, with A destroyed half way,
then on two host threads at once; every array must equal, bit for bit, what the same context produces alone.
"""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_EX = os.path.join(os.path.dirname(HERE), "examples", "idealized_geometries")
if _EX not in sys.path:
    sys.path.insert(0, _EX)

STEPS = 4


def _make():
    """The 768-tet one-axon box at P1, HH membrane with the stimulus on, block-Jacobi preconditioner only (KNP_NO_AMG set by the test)."""
    from idealized_common import make_solver, solver_parameters, Constant
    from common import small_3d
    S = make_solver(dim=3, resolution=0, n_axons=1, degree=1, mesh_tuple=small_3d())
    S._unpack_solver_params(solver_parameters(3, 0, emi_dg_chebyshev=True))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    assert not S.use_amg
    return S, Constant(0.0)


def _step(run, k):
    S, t = run
    S.step_membrane_models(k)
    S.solve_for_time_step(k, t)
    return {"emi_niter": np.asarray(S.emi_niter), "knp_niter": np.asarray(S.knp_niter).ravel(), "c": S.c.array().copy(),
            "phi": S.phi.array().copy(), "phi_M": S.phi_M_prev_PDE.array().copy(), "state": S.dev.state_save().copy()}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _maxdiff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def _blocks(blob):
    """The blocks of a snapshot as arrays, in the order of its block table (the counters too: they compare as numbers)."""
    from knpemidg import checkpoint as ck
    return ck.split_snapshot(blob)[1]


def _differing_blocks(a, b):
    return "snapshot blocks that differ: %s" % [i for i, (x, y) in enumerate(zip(_blocks(a), _blocks(b))) if not _same_bits(x, y)]


def test_interleaved_contexts_reproduce_a_lone_run(hip_lib, monkeypatch):
    monkeypatch.setenv("KNP_NO_AMG", "1")
    lone = []
    for _ in range(2):                                              # A and A'
        run = _make()
        lone.append([_step(run, k) for k in range(STEPS)])
        run[0].dev.close()
    A, A2 = lone
    exact = all(_same_bits(a[key], b[key]) for a, b in zip(A, A2) for key in a)
    yard = {key: max(_maxdiff(a[key], b[key]) for a, b in zip(A, A2)) for key in A[0] if key != "state"}
    pairs = [(_blocks(a["state"]), _blocks(b["state"])) for a, b in zip(A, A2)]
    yard_state = [max(_maxdiff(x[i], y[i]) for x, y in pairs) for i in range(len(pairs[0][0]))]
    print("yardstick A vs A' (max-norm per field):", {k: v for k, v in yard.items() if v}, "bit-identical:", exact)
    assert all(_same_bits(a[key], b[key]) for a, b in zip(A, A2) for key in ("emi_niter", "knp_niter"))
    assert np.abs(A[-1]["phi_M"] - A[0]["phi_M"]).max() > 0          # the stimulus is on: the steps differ from one another

    B, C = _make(), _make()
    got = {"B": [], "C": []}
    for who, k in (("B", 0), ("B", 1), ("C", 0), ("B", 2), ("C", 1), ("B", 3)):
        got[who].append(_step(B if who == "B" else C, k))
    B[0].dev.close()                                                # closing B must leave C stepping
    for k in (2, 3):
        got["C"].append(_step(C, k))
    C[0].dev.close()
    for who, snaps in got.items():
        assert len(snaps) == STEPS
        for k, (a, b) in enumerate(zip(A, snaps)):
            assert _same_bits(a["emi_niter"], b["emi_niter"]) and _same_bits(a["knp_niter"], b["knp_niter"]), (who, k, a["emi_niter"], b["emi_niter"])
            for key in a:
                if exact:
                    assert _same_bits(a[key], b[key]), (who, "step", k, key, _differing_blocks(a[key], b[key]) if key == "state" else "")
                elif key != "state":
                    assert _maxdiff(a[key], b[key]) <= 4.0 * yard[key], (who, "step", k, key, _maxdiff(a[key], b[key]), yard[key])
                else:
                    for i, (x, y) in enumerate(zip(_blocks(a[key]), _blocks(b[key]))):
                        assert x.shape == y.shape and _maxdiff(x, y) <= 4.0 * yard_state[i], (who, "step", k, "state block", i, _maxdiff(x, y), yard_state[i])


# ---- two contexts of different kinds through every per-context table -------------------------------------------------------------
_CASES, _LONE = {}, {}


def _case(which):
    """(problem, seeded x): "A" the jittered box of test_unstructured_apply_kernel_variants (3 456 tets, no geometry classes), "B" the
    r=0 box of make_mesh_3D (15 552 tets), the smallest one on which tests/test_gpu_parity.py asserts the structured ring variants."""
    if which not in _CASES:
        import knpemi_oracle as ko
        from common import small_3d, synthetic_state
        if which == "A":
            m, s, f = small_3d((16, 6, 6))
            rng = np.random.default_rng(11)
            inner = np.ones(m.num_vertices(), dtype=bool)
            inner[np.unique(m.facets[m.exterior_facets()])] = False
            jit = rng.uniform(-1, 1, size=m.coords.shape) * np.array([0.2e-6, 0.02e-6, 0.02e-6])
            m.coords[inner] += jit[inner]
            pb = ko.build_idealized(m, s.array(), f.array(), membrane_tags=(1,))
        else:
            from knpemidg.mesh import make_mesh_3D
            m, s, f = make_mesh_3D(0)
            pb = ko.build_idealized(m, s.array(), f.array())
        _CASES[which] = (pb, synthetic_state(pb))
    return _CASES[which]


_VARIANTS = {"A": (10, 10), "B": (3, 7)}       # (EMI, KNP): unstructured ring; structured ring (tests/test_gpu_parity.py)


def _open(which):
    from common import device_for, push_state
    pb, _ = _case(which)
    dev = device_for(pb)
    assert (dev.apply_variant(0), dev.apply_variant(1)) == _VARIANTS[which]
    push_state(dev, pb)
    dev.update_kappa(); dev.update_dnphi()
    return dev


def _leak_tables(pb, shift=0.0):
    from knpemidg.models import mm_leak
    n = len(pb.mem)
    st = np.tile(mm_leak.init_state_values(), (n, 1))
    st[:, 0] += 1e-3 * np.linspace(-1.0, 1.0, n) + shift
    pr = np.tile(mm_leak.init_parameter_values(Cm=0.02, E_Na=0.0533, E_K=-0.0936, K_e=3.32, Na_i=12.8), (n, 1))
    pr[:, mm_leak.parameter_indices("stim_amplitude")] = np.linspace(0.0, 40.0, n)
    return mm_leak.MODEL_ID, pb.mem, st, pr


def _grid_args(pb):
    lo, hi = pb.mesh.coords.min(axis=0), pb.mesh.coords.max(axis=0)
    shape = np.array([4, 3, 3])
    return lo + 0.11 * (hi - lo), 0.78 * (hi - lo) / (shape - 1), shape


def _s_apply(dev, which, out, tag=""):
    from knpemidg import _abi as A
    pb, x = _case(which)
    dev.upload(A.F_X, x[0]); dev.emi_apply(A.F_X, A.F_Y)
    out[tag + "y_emi"] = dev.download(A.F_Y, 0, pb.ndof)
    dev.upload(A.F_X, x); dev.knp_apply(A.F_X, A.F_Y)
    out[tag + "y_knp"] = dev.download(A.F_Y)


def _s_ode(dev, which, out):
    pb, _ = _case(which)
    model, facets, st, pr = _leak_tables(pb)
    h = dev.ode_create(model, facets, st, pr)
    assert h == 0
    dev.ode_step(h, 0.0, 1e-4)
    out["ode"] = dev.ode_table(h, 0, st.shape)
    assert np.abs(out["ode"] - st).max() > 0


def _s_rec(dev, which, out):
    from knpemidg import _abi as A
    pb, _ = _case(which)
    nc = pb.mesh.num_cells()
    dev.rec_create(8, [0, nc // 2], np.full((2, 4), 0.25), [0], [], [], 0, None, None)
    for k in range(3):
        dev.upload(A.F_PHI, pb.phi * (1.0 + 0.5 * k))
        dev.rec_sample(k * 1e-4)
    out["rec_t"], out["rec_rows"] = dev.rec_read()
    assert out["rec_rows"].shape == (3, 2 * (len(pb.ions) + 1)) and np.abs(out["rec_rows"][2] - out["rec_rows"][0]).max() > 0


def _s_grid(dev, which, out):
    lo, h, shape = _grid_args(_case(which)[0])
    g = dev.grid_create(lo, h, shape, [0])
    assert g == 0
    dev.grid_sample(g)
    out["frame"] = dev.grid_fetch(g, 1, 36)
    assert np.isfinite(out["frame"]).all()


def _s_save(dev, which, out, tag=""):
    out[tag + "snap"] = dev.state_save().copy()


_FIRST = (_s_apply, _s_ode, _s_rec, _s_grid, _s_save)


def _again(dev, which, out):
    """What B repeats once A is gone: the applies, a sample, a frame and a save."""
    _s_apply(dev, which, out, "2_")
    dev.rec_sample(3e-4)
    out["2_rec_t"], out["2_rec_rows"] = dev.rec_read()
    dev.grid_sample(0)
    out["2_frame"] = dev.grid_fetch(0, 1, 36)
    _s_save(dev, which, out, "2_")


def _whole(which, out):
    """The sequence from the creation of the context to its destruction, as one thread runs it."""
    dev = _open(which)
    try:
        for step in _FIRST:
            step(dev, which, out)
        if which == "B":
            _again(dev, which, out)
    finally:
        dev.close()


def _lone(which):
    if which not in _LONE:
        _LONE[which] = {}
        _whole(which, _LONE[which])
    return _LONE[which]


def _assert_equal_to_lone(which, got):
    want = _lone(which)
    assert set(got) == set(want)
    for key in want:
        g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (which, key)
        assert np.array_equal(g.reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8)), (which, key)     # bit for bit


def test_two_kinds_of_context_interleaved_on_one_thread(hip_lib):
    from knpemidg import _abi
    lone_a, lone_b = _lone("A"), _lone("B")
    a, b = _open("A"), _open("B")
    got_a, got_b = {}, {}
    try:
        for step in _FIRST:
            step(a, "A", got_a)
            step(b, "B", got_b)
        _assert_equal_to_lone("A", got_a)
        # A grows a second membrane set and a second grid: handles B does not have
        pb_a = _case("A")[0]
        ha2 = a.ode_create(*_leak_tables(pb_a, shift=1e-3))
        ga2 = a.grid_create(*_grid_args(pb_a), [0])
        assert (ha2, ga2) == (1, 1)
        with pytest.raises(_abi.KnpError, match=r"knp_grid_sample failed \(-1\): knp_grid_sample: no grid with handle 1 \(knp_grid_create\)"):
            b.grid_sample(ga2)
        with pytest.raises(_abi.KnpError, match=r"knp_grid_fetch failed \(-1\): knp_grid_fetch: no grid with handle 1 \(knp_grid_create\)"):
            b.grid_fetch(ga2, 1, 36)
        with pytest.raises(_abi.KnpError, match=r"knp_ode_step failed \(-1\)"):
            b.ode_step(ha2, 0.0, 1e-4)
        with pytest.raises(_abi.KnpError, match=r"knp_rec_add_states: channel 0, entry 0: unknown ODE handle 1"):
            b.rec_add_states([0, 1], [ha2], [0], [0], [1.0])
        a.close()                                                   # destroying A must leave B with everything it owns
        _again(b, "B", got_b)
    finally:
        a.close(); b.close()
    _assert_equal_to_lone("B", got_b)
    assert lone_a["snap"].size != lone_b["snap"].size


def test_two_kinds_of_context_on_two_threads(hip_lib):
    """Thread 1 drives A, thread 2 drives B, from knp_ctx_create to knp_ctx_destroy, started together.  One run, nothing compiled at
    run time inside the threads; a thread that does not come back fails the test."""
    _lone("A"); _lone("B")                                          # the references (and the problems) exist before the threads start
    barrier = threading.Barrier(2)
    got, errors = {"A": {}, "B": {}}, []

    def run(which):
        try:
            barrier.wait(timeout=60)
            _whole(which, got[which])
        except BaseException as e:                                  # reported by the main thread
            errors.append((which, repr(e)))

    threads = [threading.Thread(target=run, args=(w,), daemon=True) for w in ("A", "B")]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a context's thread did not finish"
    assert not errors, errors
    _assert_equal_to_lone("A", got["A"])
    _assert_equal_to_lone("B", got["B"])
