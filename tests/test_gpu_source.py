"""Ion sources evaluated on the device (knpemidg.Expression -> csrc/source_rtc.hpp, csrc/source.hip): the load-vector rows against
the host rule (mms_terms._cell_source on a hand-written numpy twin, tests/source_cases.py), tails of the cell list, ghost cells of
a partition, idempotence, parameters without recompiles, host round trips, the KNP right-hand side against the oracle, host and
device sources side by side, refusals, checkpoint / resume and the tortuosity example.

Bound of every row comparison: |device - host| <= 1e-12 * scale per entry, scale = vol sum_q w_q |f(x_q)| |B[q][a]| (source_cases.BOUND:
125 terms with a few roundings each ~ 2e-14; sin differs by an ulp or two between the device and numpy).  Each test prints the worst
ratio it saw."""
import os
import sys

import numpy as np
import pytest

import knpemi_oracle as ko
from common import device_for, relerr, set_params_of, small_3d

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "examples", "idealized_geometries"), os.path.join(ROOT, "examples", "emix_simulations"),
           os.path.join(ROOT, "examples", "local_astrocyte_depolarization")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import source_cases as SC                              # noqa: E402


def _device(name, degree, tags=None, **kw):
    from knpemidg import _abi as A
    mesh, sub, surf = SC.mesh_of(name)
    tags = sub.array() if tags is None else tags
    return A.Device(mesh, tags, surf.array(), (1, 2) if name == "emix_sub" else (1,), 3, degree=degree, **kw), mesh, np.asarray(tags)


def _check_row(got, mesh, tags, degree, f, t, what):
    row, scale = SC.host_row(mesh, tags, degree, f, t)
    ratio = SC.worst_ratio(got, row, scale)
    print("%s: worst |device - host| / scale = %.3e (bound %.0e), entries with scale > 0: %d" % (what, ratio, SC.BOUND, int((scale > 0).sum())))
    assert ratio <= SC.BOUND, (what, ratio)
    return row


# --------------------------------------------------------------------------------------------------------- 1. row against the host rule
@pytest.mark.parametrize("name,degree", SC.ROW_CASES)
def test_row_matches_host_rule_inside_and_outside_the_window(hip_lib, name, degree):
    from knpemidg import Constant
    dev, mesh, tags = _device(name, degree)
    try:
        if name == "emix_sub":
            assert not np.array_equal(dev.cell_order, np.arange(dev.nc)) and len(np.unique(tags)) == 3
        t = Constant(SC.T_IN)
        expr = SC.expression(mesh, t)
        dev.source_register(0, expr)
        assert dev.source_cells() == int((tags == 0).sum())
        dev.source_eval(0, expr.values())
        got = dev.source_download()
        assert got.shape == (2, mesh.num_cells(), dev.nd)
        row = _check_row(got[0], mesh, tags, degree, SC.twin(mesh), SC.T_IN, "%s P%d" % (name, degree))
        assert np.abs(row).max() > 0
        assert np.all(got[0][tags != 0] == 0.0)                    # non-ECS cells: exactly zero
        assert np.all(got[1] == 0.0)                               # the other species' row: exactly zero
        t.assign(SC.T_OUT)
        dev.source_eval(0, expr.values())
        assert np.all(dev.source_download() == 0.0)                # outside the window: exactly zero
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------- 2. tails
@pytest.mark.parametrize("length", [0, 1, 63, 64, 65])
def test_tail_of_the_cell_list(hip_lib, length):
    """ECS lists of length 0, 1, 63, 64, 65 (one lane per cell, 64 lanes per block) by retagging cells of small_3d(); the lengths that
    are no multiple of the block size in general are those of the meshes above (672, 312, 66 and 10 468 cells).  An empty list launches
    nothing: a launch of zero blocks would be refused by the runtime, and the evaluation succeeds."""
    mesh, sub, _ = SC.mesh_of("small_3d")
    f = SC.twin(mesh)
    _, scale = SC.host_row(mesh, sub.array(), 1, f, SC.T_IN)
    ecs = np.nonzero(sub.array() == 0)[0]
    ecs = ecs[np.argsort(~(scale[ecs].max(axis=1) > 0), kind="stable")]        # the cells the box touches first
    tags = np.array(sub.array(), copy=True)
    tags[ecs[length:]] = 1
    dev, mesh, tags = _device("small_3d", 1, tags=tags)
    try:
        expr = SC.expression(mesh, SC.T_IN)
        dev.source_register(1, expr)
        assert dev.source_cells() == length == int((tags == 0).sum())
        dev.source_eval(1, expr.values())
        got = dev.source_download()
        row = _check_row(got[1], mesh, tags, 1, f, SC.T_IN, "list of %d" % length)
        assert (np.abs(row).max() > 0) == (length > 0) and np.all(got[0] == 0.0)
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------- 3. ghost cells
def test_ghost_cells_of_a_partition_carry_the_row(hip_lib):
    """Rank 0 of a two-slab partition, built in one process without a communicator (as tests/test_gpu_recorder_partition.py does):
    the row equals the host rule on the local mesh on owned and ghost ECS cells.  The box is the global mesh's: it crosses the cut."""
    from knpemidg.partition import Partition
    m, s, f = SC.mesh_of("small_3d_844")
    loc = Partition(m, 2, method="slab").local(0)
    sub_l, surf_l = loc.localize(s, f, (1,))
    pb = ko.build_idealized(loc.mesh, sub_l.array(), surf_l.array(), membrane_tags=(1,))
    dev = device_for(pb, nc_owned=loc.nc_owned)
    try:
        tags = np.asarray(sub_l.array())
        expr = SC.expression(m, SC.T_IN)
        dev.source_register(0, expr)
        dev.source_eval(0, expr.values())
        got = dev.source_download()
        row = _check_row(got[0], loc.mesh, tags, 1, SC.twin(m), SC.T_IN, "partition rank 0")
        ghost = np.arange(loc.mesh.num_cells()) >= loc.nc_owned
        assert ghost.any() and np.abs(row[ghost]).max() > 0 and np.abs(row[~ghost]).max() > 0
        assert dev.source_cells() == int((tags == 0).sum()) > int((tags[~ghost] == 0).sum())
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------- 4. idempotence, parameters, round trips
def test_idempotent_parameters_without_recompile_and_no_round_trips(hip_lib, monkeypatch):
    from knpemidg import ode_rtc
    dev, mesh, tags = _device("small_3d", 1)
    try:
        expr = SC.expression(mesh, SC.T_IN)
        dev.source_register(0, expr)
        calls = []
        real = ode_rtc._hiprtc
        monkeypatch.setattr(ode_rtc, "_hiprtc", lambda src, kernel: (calls.append(kernel), real(src, kernel))[1])
        dev.source_eval(0, expr.values())
        first = dev.source_download()
        rt = dev.host_round_trips()
        dev.source_eval(0, expr.values())
        assert dev.host_round_trips() == rt                        # an evaluation neither waits nor copies
        second = dev.source_download()
        assert first.tobytes() == second.tobytes() and np.abs(first[0]).max() > 0
        expr.g = 2.0 * SC.G
        rt = dev.host_round_trips()
        dev.source_register(0, expr)                               # same kernel: left alone (no compile, no unload, no stream drain)
        assert dev.host_round_trips() == rt
        dev.source_eval(0, expr.values())
        doubled = dev.source_download()
        _check_row(doubled[0], mesh, tags, 1, SC.twin(mesh, g=2.0 * SC.G), SC.T_IN, "g doubled")
        assert np.array_equal(doubled[0], 2.0 * first[0])          # a factor of two is exact in binary
        assert calls == []
        # another expression on the same species replaces its kernel (one compile)
        from knpemidg import Expression
        half = Expression("0.5 * (" + SC.code(3) + ")", **SC.params(mesh, SC.T_IN, g=2.0 * SC.G))
        dev.source_register(0, half)
        dev.source_eval(0, half.values())
        assert len(calls) == 1 and np.array_equal(dev.source_download()[0], first[0])
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------- 5. end to end against the oracle
@pytest.mark.parametrize("dim,degree", [(2, 1), (3, 1), (2, 2)])
def test_expression_and_array_sources_vs_oracle(hip_lib, dim, degree):
    """The procedure of tests/test_gpu_solver.py::test_f_source_array_and_callable_vs_oracle with the callable replaced by an
    Expression on the device side and by its numpy twin on the oracle side: L_knp inside and outside the window at 1e-11 of the
    total and 1e-6 of the source's own contribution; a whole _update_sources makes no host round trip."""
    from idealized_common import make_solver, solver_parameters, Constant
    from knpemidg import _abi as A
    mt = None if dim == 2 else small_3d()          # make_mesh_2D(0) and small_3d(): the meshes of source_cases "mesh_2d" / "small_3d"
    S = make_solver(dim=dim, resolution=0, n_axons=1, degree=degree, mesh_tuple=mt)
    mesh = S.mesh
    t = Constant(0.0)
    rng = np.random.default_rng(8)
    per_cell = rng.uniform(-5.0, 5.0, mesh.num_cells())
    pb = ko.build_idealized(mesh, S.subdomains.array(), S.surfaces.array(), p=degree, membrane_tags=(1,))
    S.ion_list[0]['f_source'] = SC.expression(mesh, t)
    S.ion_list[1]['f_source'] = per_cell
    S._unpack_solver_params(solver_parameters(dim, 0))
    S.splitting_scheme = True
    S.setup_varform_emi()
    assert list(S._device_sources) == [0] and not S._callable_sources
    S.step_membrane_models(0)                      # identical inputs on both sides: the oracle takes the device's state
    nf = mesh.num_facets()
    pb.c = S.c.array().reshape(pb.c.shape); pb.c_prev_n = S.c_prev_n.array().reshape(pb.c.shape)
    pb.c_elim = S.ion_list[-1]['c'].array().reshape(pb.c_elim.shape); pb.phi = S.phi.array().reshape(pb.phi.shape)
    pb.phi_M = S.phi_M_prev_PDE.array().copy()
    Ich = S.dev.download(A.F_I_CH).reshape(3, nf)
    for k, ion in enumerate(pb.ions):
        pb.I_ch[ion["name"]] = Ich[k].copy()
    base = [ko.knp_rhs(pb, k) for k in range(2)]
    pb.f_source = [SC.twin(mesh), per_cell]
    for tt, active in ((SC.T_OUT, False), (SC.T_IN, True)):
        t.assign(tt)                               # the Expression follows the time constant, as in solve_for_time_step
        rt = S.dev.host_round_trips()
        S._update_sources(tt)
        assert S.dev.host_round_trips() == rt
        pb.t = tt
        S.dev.knp_rhs()
        got = S.dev.download(A.F_B_KNP).reshape(2, -1)
        for k in range(2):
            ref = ko.knp_rhs(pb, k).ravel()
            print("dim %d P%d t %g species %d: relerr total %.3e" % (dim, degree, tt, k, relerr(got[k], ref)))
            assert relerr(got[k], ref) < 1e-11
            d_ref = ref - base[k].ravel()
            assert (np.abs(d_ref).max() > 0) == (active or k == 1)
            if np.abs(d_ref).max() > 0:          # the source is 1e-3 ... 1e-5 of the mass term: 1e-11 of the total = 1e-6 of its own size
                assert relerr(got[k] - base[k].ravel(), d_ref) < 1e-6
    S.dev.close()


# --------------------------------------------------------------------------------------------------------- 6. host and device sources together
def test_host_callable_and_expression_side_by_side(hip_lib, monkeypatch):
    from idealized_common import make_solver, solver_parameters, Constant
    S = make_solver(dim=3, resolution=0, n_axons=1, mesh_tuple=small_3d())
    mesh, tags = S.mesh, np.asarray(S.subdomains.array())
    t = Constant(0.0)
    f1 = SC.twin(mesh, g=-15.0)
    S.ion_list[0]['f_source'] = SC.expression(mesh, t)
    S.ion_list[1]['f_source'] = lambda X, tt: f1(X, tt)
    S._unpack_solver_params(solver_parameters(3, 0))
    S.splitting_scheme = True
    S.setup_varform_emi()
    assert list(S._device_sources) == [0] and list(S._callable_sources) == [1]
    # pushing the parameters again with the same Expression loads no module again
    loads = []
    real = S.dev.lib.knp_source_register
    monkeypatch.setattr(S.dev.lib, "knp_source_register", lambda *a: (loads.append(a[1]), real(*a))[1])
    S._push_params(True)
    assert loads == [] and list(S._device_sources) == [0]
    monkeypatch.undo()
    for tt in (SC.T_IN, SC.T_OUT, SC.T_IN):                        # two consecutive updates at different t leave no stale row
        t.assign(tt)
        S._update_sources(tt)
        got = S.dev.source_download()
        r0 = _check_row(got[0], mesh, tags, 1, SC.twin(mesh), tt, "device row, t = %g" % tt)
        r1 = _check_row(got[1], mesh, tags, 1, f1, tt, "host row, t = %g" % tt)
        assert (np.abs(r0).max() > 0) == (np.abs(r1).max() > 0) == (tt == SC.T_IN)
    S.dev.close()


# --------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_clear_and_free(hip_lib):
    from knpemidg import _abi as A
    mesh, sub, surf = SC.mesh_of("small_3d")
    expr = SC.expression(mesh, SC.T_IN)
    kernel, code = expr.compiled(3, 4)
    n = len(expr.names)

    def raw(dev, species, n_params):
        rc = dev.lib.knp_source_register(dev.ctx, species, code, len(code), kernel.encode(), n_params)
        return rc, dev.lib.knp_last_error(dev.ctx).decode()
    pb = ko.build_idealized(mesh, sub.array(), surf.array(), membrane_tags=(1,))
    dev = device_for(pb)
    try:
        dev.source_register(0, expr)                               # rule, cell list and buffer exist from here on
        rc, why = raw(dev, dev.n_sys, n)
        assert rc == -1 and "species" in why
        rc, why = raw(dev, -1, n)
        assert rc == -1 and "species" in why
        rc, why = raw(dev, 1, 33)
        assert rc == -1 and "parameters" in why
        assert raw(dev, 1, 32)[0] == 0                             # 32 is allowed; the count is checked again at the evaluation
        with pytest.raises(A.KnpError, match="parameter count"):
            dev.source_eval(1, expr.values())
        with pytest.raises(A.KnpError, match="no source registered"):
            dev.source_eval(2, expr.values())
        dev.source_eval(0, expr.values())
        assert np.abs(dev.source_download()[0]).max() > 0
        dev.set_source(None)                                       # with device sources registered: zeroed, not freed
        assert np.all(dev.source_download() == 0.0)
        dev.source_eval(0, expr.values())
        dev.source_clear(0)
        assert np.all(dev.source_download()[0] == 0.0)
        with pytest.raises(A.KnpError, match="no source registered"):
            dev.source_eval(0, expr.values())
        dev.source_clear(1)
        dev.set_source(None)                                       # no device source left: frees, as before
        assert dev.source_download() is None
        # manufactured-solution mode owns the buffer
        nc, nd = mesh.num_cells(), dev.nd
        dev.set_mms(np.zeros((2, nc)), np.zeros((nc, nd)), np.zeros((2, nc, nd)))
        pb.splitting = 2
        set_params_of(dev, pb)
        rc, why = raw(dev, 0, n)
        assert rc == -1 and "manufactured" in why
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------- 8. resume
def _resume_solver(t):
    from idealized_common import make_solver, solver_parameters
    mt = small_3d()
    S = make_solver(dim=3, resolution=0, n_axons=1, mesh_tuple=mt)
    # on for 1.5e-4 <= t <= 3.5e-4: steps 2 and 3 (t = 2e-4, 3e-4), the ones behind the checkpoint
    from knpemidg import Expression
    S.ion_list[0]['f_source'] = Expression(SC.code(3), degree=4, **dict(SC.params(S.mesh, t), t0=1.5e-4, t1=3.5e-4))
    S._unpack_solver_params(solver_parameters(3, 0, emi_dg_chebyshev=True))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    return S


def _steps(S, t, k0, k1):
    snaps = []
    for k in range(k0, k1):
        S.step_membrane_models(k)
        S.solve_for_time_step(k, t)
        snaps.append({"c": S.c.array().copy(), "c_elim": S.ion_list[-1]['c'].array().copy(), "phi": S.phi.array().copy(),
                      "src": np.abs(S.dev.source_download()[0]).max()})
    return snaps


def test_resume_with_an_expression_source(hip_lib, tmp_path, monkeypatch):
    """2 steps, checkpoint, a new solver resumed for 2 more with the source on in steps 2 and 3, against 4 steps straight.  The
    comparison is the one of tests/test_gpu_checkpoint.py::test_resume_is_bit_exact (lines 183-211 there): two uninterrupted runs
    measure the yardstick; bit for bit if they agree bit for bit, else within four times their difference.  No new state is
    checkpointed: the row is recomputed before every KNP solve from t, which load_checkpoint sets."""
    from idealized_common import Constant
    monkeypatch.setenv("KNP_NO_AMG", "1")
    runs = []
    for _ in range(2):
        t = Constant(0.0)
        S = _resume_solver(t)
        runs.append(_steps(S, t, 0, 4))
        S.dev.close()
    A, A2 = runs
    assert [s["src"] > 0 for s in A] == [False, False, True, True]
    keys = ("c", "c_elim", "phi")
    yard = {key: max(float(np.abs(a[key] - b[key]).max()) for a, b in zip(A, A2)) for key in keys}
    exact = all(a[key].tobytes() == b[key].tobytes() for a, b in zip(A, A2) for key in keys)
    print("yardstick A vs A':", yard, "bit-identical:", exact)
    path = str(tmp_path / "ck.h5")
    t = Constant(0.0)
    B1 = _resume_solver(t)
    _steps(B1, t, 0, 2)
    B1.save_checkpoint(path)
    B1.dev.close()
    del B1
    t = Constant(0.0)
    B2 = _resume_solver(t)
    assert B2.load_checkpoint(path, t=t) == 2 and abs(float(t) - 2.0e-4) < 1e-18
    B = _steps(B2, t, 2, 4)
    B2.dev.close()
    assert [s["src"] > 0 for s in B] == [True, True]
    for j, b in enumerate(B):
        a = A[2 + j]
        for key in keys:
            diff = float(np.abs(a[key] - b[key]).max())
            if exact:
                assert a[key].tobytes() == b[key].tobytes(), ("step", 3 + j, key, diff)
            else:
                assert diff <= 4.0 * yard[key], ("step", 3 + j, key, diff, yard[key])


# --------------------------------------------------------------------------------------------------------- 9. the example
def test_tortuosity_example_runs_and_the_source_moves_potassium(hip_lib):
    """examples/local_astrocyte_depolarization/run_tortuosity.py, baseline variant, on the bundled reconstruction.  The source is on
    from t = 0.2 ms, so three steps are taken (t = 0, 0.1, 0.2 ms at the KNP solves): steps 0 and 1 lie before the window, step 2 in
    it.  K in the box (source +g) rises and Na (source -g) falls in that step, by more than either moved in the steps before it."""
    import run_tortuosity as RT
    h = RT.main(steps=3, variant="baseline")
    S = h["solver"]
    try:
        assert np.isfinite(S.c.array()).all() and np.isfinite(S.phi.array()).all() and np.isfinite(S.ion_list[-1]['c'].array()).all()
        assert sorted(S._device_sources) == [0, 1] and not S._callable_sources
        # the mesh is tagged 1 glial / 2 neuronal, the oracle's tuples 1 neuronal / 2 glial: glial cells start at the glial K
        init_K = ko.tortuosity_params()["init"]["K"]
        assert init_K[2] < 100.0 < init_K[1]                       # (ECS, neuronal 124.14, glial 99.31)
        # means of constant fields over up to 5e5 values: pairwise summation, a few eps log2(n) ~ 1e-14
        assert np.allclose(h["K_init_by_subdomain"], [init_K[0], init_K[2], init_K[1]], rtol=1e-13, atol=0.0)
        rho, tags = ko.tortuosity_params()["rho"], np.asarray(S.subdomains.array())
        for s, col in enumerate((0, 2, 1)):
            assert np.all(np.asarray(S.rho)[tags == s] == rho[col])
        K, Na = np.asarray(h["K_box"]), np.asarray(h["Na_box"])
        dK, dNa = np.diff(K), np.diff(Na)
        print("K in the box:", K, "Na in the box:", Na)
        assert dK[2] > 0 and dNa[2] < 0
        assert dK[2] > np.abs(dK[:2]).max() and -dNa[2] > np.abs(dNa[:2]).max()
    finally:
        S.dev.close()
