"""Ion sources that read phi and the concentrations, on any subdomain (knpemidg.FieldExpression -> csrc/source_rtc.hpp,
csrc/source.hip): rows against hand-written numpy twins (tests/field_source_cases.py), one-hot rows against the host mass matrix,
subdomain selections and list tails, re-registration, the time level the solver evaluates at, the global balance of an injected
species, a partition's rank, checkpoint / resume, refusals, two contexts, and the uptake example.

Bound of every row comparison: |device - twin| <= 1e-12 * scale per entry (field_source_cases.BOUND), scale built from the sum of the
absolute values of the terms of f.  Each test prints the worst ratio it saw."""
import os
import sys

import numpy as np
import pytest

import knpemi_oracle as ko
from common import device_for, set_params_of, small_3d

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "examples", "idealized_geometries"), os.path.join(ROOT, "examples", "emix_simulations")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import field_source_cases as FC                        # noqa: E402
import source_cases as SC                              # noqa: E402


def _device(name, degree, tags=None, **kw):
    from knpemidg import _abi as A
    mesh, sub, surf = SC.mesh_of(name)
    tags = sub.array() if tags is None else tags
    dev = A.Device(mesh, tags, surf.array(), (1, 2) if name == "emix_sub" else (1,), len(FC.IONS), degree=degree, **kw)
    U = FC.fields(mesh.num_cells(), dev.nd)
    FC.upload(dev, U)
    return dev, mesh, np.asarray(tags), U


def _check(got, row, scale, what):
    ratio = FC.worst_ratio(got, row, scale)
    print("%s: worst |device - twin| / scale = %.3e (bound %.0e), entries with scale > 0: %d" % (what, ratio, FC.BOUND, int((scale > 0).sum())))
    assert ratio <= FC.BOUND, (what, ratio)
    return row


def _eval(dev, species, expr):
    dev.source_eval(species, expr.values())
    return dev.source_download()


# --------------------------------------------------------------------------------------------------------- 1. rows against the twin
@pytest.mark.parametrize("name,degree", SC.ROW_CASES)
def test_rows_match_the_twin_inside_and_outside_the_window(hip_lib, name, degree):
    """NF = 1 (linear), 2 (nonlinear) and n_ions + 1 on every mesh and basis of the plain-source tests."""
    from knpemidg import Constant
    dev, mesh, tags, U = _device(name, degree)
    try:
        if name == "emix_sub":
            assert not np.array_equal(dev.cell_order, np.arange(dev.nc)) and len(np.unique(tags)) == 3
        for case in (FC.LINEAR, FC.NONLINEAR, FC.ALL_FIELDS):
            t = Constant(FC.T_IN)
            expr = case.expression(t)
            dev.source_register(0, expr, ion_names=FC.IONS)
            assert dev.source_cells() == -1                            # the shared ECS list belongs to plain sources: not built
            got = _eval(dev, 0, expr)
            assert got.shape == (2, mesh.num_cells(), dev.nd)
            row = _check(got[0], *FC.twin_row(mesh, tags, degree, case, U, FC.T_IN), "%s P%d %s" % (name, degree, case.name))
            assert np.all(np.abs(row[tags == 0]).max(axis=1) > 0)
            assert np.all(got[0][tags != 0] == 0.0) and np.all(got[1] == 0.0)
            t.assign(FC.T_OUT)
            assert np.all(_eval(dev, 0, expr) == 0.0)                  # outside the window: exactly zero
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------- 2. one field at a time
@pytest.mark.parametrize("name,degree", SC.ROW_CASES)
def test_one_hot_rows_are_the_mass_matrix_product_of_that_field(hip_lib, name, degree):
    """code = "<name>" for phi and every ion in turn, the eliminated one included: the row is the cell mass matrix applied to that
    field's nodal values and to no other's, on every mesh of test 1 (the EMIx submesh has a permuted device cell order)."""
    from knpemidg import FieldExpression
    dev, mesh, tags, U = _device(name, degree)
    try:
        for fname in FC.FIELD_NAMES:
            expr = FieldExpression(fname, fields=(fname,))
            dev.source_register(1, expr, ion_names=FC.IONS)
            got = _eval(dev, 1, expr)
            row, scale = FC.mass_row(mesh, tags, degree, U[fname])
            _check(got[1], row, scale, "%s P%d one-hot %s" % (name, degree, fname))
            others = [FC.worst_ratio(got[1], FC.mass_row(mesh, tags, degree, U[o])[0], scale) for o in FC.FIELD_NAMES if o != fname]
            assert min(others) > 1e-3 and np.all(got[0] == 0.0)        # no other field passes for it
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------- 3. subdomains and tails
def test_subdomain_selections_and_an_absent_tag(hip_lib):
    dev, mesh, tags, U = _device("small_3d", 1)
    try:
        case = FC.NONLINEAR
        for subdomains in ((0,), (1,), (0, 1), (1, 0), (7,), (7, 1)):
            expr = case.expression(FC.T_IN, subdomains=subdomains)
            dev.source_register(0, expr, ion_names=FC.IONS)
            rt = dev.host_round_trips()
            dev.source_eval(0, expr.values())                          # an absent tag: nothing launched, the call succeeds
            assert dev.host_round_trips() == rt
            got = dev.source_download()
            row = _check(got[0], *FC.twin_row(mesh, tags, 1, case, U, FC.T_IN, subdomains), "subdomains %r" % (subdomains,))
            inside = np.isin(tags, subdomains)
            assert np.all(got[0][~inside] == 0.0) and np.all(np.abs(row[inside]).max(axis=1) > 0) and np.all(got[1] == 0.0)
            assert inside.any() == (subdomains != (7,))
    finally:
        dev.close()


@pytest.mark.parametrize("length", [0, 1, 63, 64, 65])
def test_tail_of_the_kernels_own_cell_list(hip_lib, length):
    """Lists of 0, 1, 63, 64 and 65 cells (one lane per cell, 64 lanes per block) by retagging ECS cells of small_3d() to 2; the list
    of tag 0 has `length` cells, the list of tag 2 the rest, and (0, 2) the whole ECS again."""
    mesh, sub, _ = SC.mesh_of("small_3d")
    tags = np.array(sub.array(), copy=True)
    ecs = np.nonzero(tags == 0)[0]
    ecs = ecs[np.random.default_rng(3).permutation(len(ecs))]          # scattered over the mesh, not a prefix of the device order
    tags[ecs[length:]] = 2
    dev, mesh, tags, U = _device("small_3d", 1, tags=tags)
    try:
        assert int((tags == 0).sum()) == length
        for subdomains in ((0,), (2,), (0, 2)):
            expr = FC.ALL_FIELDS.expression(FC.T_IN, subdomains=subdomains)
            dev.source_register(1, expr, ion_names=FC.IONS)
            got = _eval(dev, 1, expr)
            row = _check(got[1], *FC.twin_row(mesh, tags, 1, FC.ALL_FIELDS, U, FC.T_IN, subdomains), "list of %d, %r" % (length, subdomains))
            inside = np.isin(tags, subdomains)
            assert int(inside.sum()) == {(0,): length, (2,): len(ecs) - length, (0, 2): len(ecs)}[subdomains]
            assert np.all(got[1][~inside] == 0.0) and np.all(np.abs(row[inside]).max(axis=1) > 0) and np.all(got[0] == 0.0)
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------- 4. re-registration
def test_reregistration_leaves_zeros_other_rows_alone_and_compiles_nothing_new(hip_lib, monkeypatch):
    from knpemidg import ode_rtc
    dev, mesh, tags, U = _device("small_3d", 1)
    try:
        plain = SC.expression(mesh, SC.T_IN)                           # species 1 holds a plain Expression throughout
        dev.source_register(1, plain)
        other = _eval(dev, 1, plain)[1].copy()
        assert np.abs(other).max() > 0 and dev.source_cells() == int((tags == 0).sum())

        def others_untouched():
            assert dev.source_download()[1].tobytes() == other.tobytes()
        # (0,) then (1,) on one species: exact zeros on the ECS
        e0 = FC.LINEAR.expression(FC.T_IN, subdomains=(0,))
        dev.source_register(0, e0, ion_names=FC.IONS)
        first = _eval(dev, 0, e0)[0].copy()
        _check(first, *FC.twin_row(mesh, tags, 1, FC.LINEAR, U, FC.T_IN, (0,)), "(0,)")
        others_untouched()
        calls = []
        real = ode_rtc._hiprtc
        monkeypatch.setattr(ode_rtc, "_hiprtc", lambda src, kernel: (calls.append(kernel), real(src, kernel))[1])
        e1 = FC.LINEAR.expression(FC.T_IN, subdomains=(1,))
        assert e1.kernel_name(3, 4) == e0.kernel_name(3, 4)
        dev.source_register(0, e1, ion_names=FC.IONS)
        assert np.all(dev.source_download()[0] == 0.0)                 # zeroed by the registration itself
        got = _eval(dev, 0, e1)[0]
        _check(got, *FC.twin_row(mesh, tags, 1, FC.LINEAR, U, FC.T_IN, (1,)), "(0,) then (1,)")
        assert np.all(got[tags == 0] == 0.0) and np.abs(got[tags == 1]).max() > 0
        others_untouched()
        e0.subdomains = (0, 1)                                         # the same object with other subdomains: a new list, no compile
        dev.source_register(0, e0, ion_names=FC.IONS)
        _check(_eval(dev, 0, e0)[0], *FC.twin_row(mesh, tags, 1, FC.LINEAR, U, FC.T_IN, (0, 1)), "(0, 1)")
        assert calls == []
        # registering the same thing again is left alone: no module load, no stream drain
        loads = []
        real_reg = dev.lib.knp_source_register_fields
        monkeypatch.setattr(dev.lib, "knp_source_register_fields", lambda *a: (loads.append(a[1]), real_reg(*a))[1])
        rt = dev.host_round_trips()
        dev.source_register(0, e0, ion_names=FC.IONS)
        assert loads == [] and dev.host_round_trips() == rt
        # evaluations make no round trip
        for _ in range(3):
            dev.source_eval(0, e0.values())
        assert dev.host_round_trips() == rt
        others_untouched()
        # Expression -> FieldExpression -> Expression on species 0: the first rows again, bit for bit
        dev.source_register(0, plain)
        a = _eval(dev, 0, plain)[0].copy()
        assert a.tobytes() == other.tobytes()                          # the same expression as species 1 holds
        dev.source_register(0, e1, ion_names=FC.IONS)
        mid = _eval(dev, 0, e1)[0]
        assert np.all(mid[tags == 0] == 0.0) and np.abs(mid[tags == 1]).max() > 0
        dev.source_register(0, plain)
        assert np.all(dev.source_download()[0] == 0.0)                 # the cells of tag 1 do not keep the field source's values
        b = _eval(dev, 0, plain)[0]
        assert a.tobytes() == b.tobytes() and np.all(b[tags != 0] == 0.0)
        others_untouched()
        assert calls == []
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------- 5. time level
def _solver(sources, **extra):
    from idealized_common import make_solver, solver_parameters
    S = make_solver(dim=3, resolution=0, n_axons=1, mesh_tuple=small_3d())
    for k, f in sources.items():
        S.ion_list[k]['f_source'] = f
    S._unpack_solver_params(solver_parameters(3, 0, **extra))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    return S


SOLVER_IONS = ("K", "Cl", "Na")                                        # idealized_common: Na is eliminated


def _solver_fields(S, c_prev, c_elim, phi):
    nc, nd = S.mesh.num_cells(), S.nd
    c_prev = np.asarray(c_prev).reshape(2, nc, nd)
    return {"c_K": c_prev[0], "c_Cl": c_prev[1], "c_Na": np.asarray(c_elim).reshape(nc, nd), "phi": np.asarray(phi).reshape(nc, nd)}


def test_time_level_of_a_step(hip_lib):
    """Two steps with the clearance source on K and a source reading phi and every ion on Cl.  The rows of the second step equal the
    twins on the concentrations downloaded BEFORE that step (level n; the eliminated ion too) and on the phi downloaded after it
    (the EMI solve of that step): not on the concentrations the step produced."""
    from idealized_common import Constant
    from knpemidg import _abi as A
    small = FC.Case("small", "1e-3 * (%s)" % FC.ALL_FIELDS.code, FC.ALL_FIELDS.fields, FC.ALL_FIELDS.params,
                    lambda X, u: 1e-3 * FC.ALL_FIELDS._f(X, u), lambda X, u: 1e-3 * FC.ALL_FIELDS._M(X, u))
    S = _solver({0: FC.LINEAR.expression(None), 1: small.expression(None)})
    try:
        assert sorted(S._device_sources) == [0, 1] and not S._callable_sources
        t = Constant(0.0)
        tags = np.asarray(S.subdomains.array())
        S.step_membrane_models(0); S.solve_for_time_step(0, t)
        c_prev, c_elim = S.dev.download(A.F_C_PREV), S.dev.download(A.F_C_ELIM)
        S.step_membrane_models(1); S.solve_for_time_step(1, t)
        U = _solver_fields(S, c_prev, c_elim, S.dev.download(A.F_PHI))
        got = S.dev.source_download()
        _check(got[0], *FC.twin_row(S.mesh, tags, 1, FC.LINEAR, U, None), "clearance, step 2")
        _check(got[1], *FC.twin_row(S.mesh, tags, 1, small, U, None), "all fields, step 2")
        after = _solver_fields(S, S.dev.download(A.F_C_PREV), S.dev.download(A.F_C_ELIM), U["phi"])
        row, scale = FC.twin_row(S.mesh, tags, 1, FC.LINEAR, after, None)
        assert FC.worst_ratio(got[0], row, scale) > 1e3 * FC.BOUND       # the level the step produced is told apart
    finally:
        S.dev.close()


def test_time_level_of_a_picard_step(hip_lib):
    """solve_for_time_step_picard with the clearance source: every iteration of the second step writes the same row, the twin's on
    the level-n concentrations."""
    from idealized_common import Constant
    from knpemidg import _abi as A
    S = _solver({0: FC.LINEAR.expression(None)})
    try:
        t = Constant(0.0)
        tags = np.asarray(S.subdomains.array())
        S.step_membrane_models(0); S.solve_for_time_step_picard(0, t)
        c_prev, c_elim = S.dev.download(A.F_C_PREV), S.dev.download(A.F_C_ELIM)
        rows = []
        real = S.dev.source_eval
        S.dev.source_eval = lambda k, v: (real(k, v), rows.append(S.dev.source_download()[0].copy()))[0]
        S.step_membrane_models(1); S.solve_for_time_step_picard(1, t)
        S.dev.source_eval = real
        print("Picard iterations of the second step: %d" % len(rows))
        assert len(rows) == S.picard_iters[-1] >= 2
        assert all(r.tobytes() == rows[0].tobytes() for r in rows[1:])
        U = _solver_fields(S, c_prev, c_elim, S.dev.download(A.F_PHI))
        _check(rows[0], *FC.twin_row(S.mesh, tags, 1, FC.LINEAR, U, None), "clearance, Picard step 2")
    finally:
        S.dev.close()


def test_picard_step_with_a_source_reading_the_eliminated_ion(hip_lib):
    """What the documentation says of the eliminated ion under Picard: knp_picard_updates recomputes KNP_F_C_ELIM from the iterate,
    so a source reading c_Na follows it.  Each iteration's row is the twin's on the KNP_F_C_ELIM downloaded right in front of that
    evaluation, and the rows of two iterations differ."""
    from idealized_common import Constant
    from knpemidg import _abi as A
    case = FC.Case("elim", "k_x * (c_Na - c0)", ("c_Na",), dict(k_x=0.5, c0=FC.C0_NA),
                   lambda X, u: 0.5 * (u["c_Na"] - FC.C0_NA), lambda X, u: 0.5 * (np.abs(u["c_Na"]) + FC.C0_NA))
    S = _solver({0: case.expression(None)})
    try:
        t = Constant(0.0)
        tags = np.asarray(S.subdomains.array())
        S.step_membrane_models(0); S.solve_for_time_step_picard(0, t)
        seen = []
        real = S.dev.source_eval

        def spy(k, v):
            c_elim = S.dev.download(A.F_C_ELIM)
            real(k, v)
            seen.append((c_elim, S.dev.source_download()[0].copy()))
        S.dev.source_eval = spy
        S.step_membrane_models(1); S.solve_for_time_step_picard(1, t)
        S.dev.source_eval = real
        assert len(seen) == S.picard_iters[-1] >= 2
        zeros = np.zeros(2 * S.mesh.num_cells() * S.nd)
        for j, (c_elim, row) in enumerate(seen):
            U = _solver_fields(S, zeros, c_elim, zeros[:len(c_elim)])
            _check(row, *FC.twin_row(S.mesh, tags, 1, case, U, None), "eliminated ion, Picard iteration %d" % (j + 1))
        assert seen[0][1].tobytes() != seen[1][1].tobytes()
    finally:
        S.dev.close()


# --------------------------------------------------------------------------------------------------------- 6. global balance
def _integral(S, species):
    X = S.mesh.coords[S.mesh.cells]
    vol = np.abs(np.linalg.det(X[:, 1:] - X[:, :1])) / 6.0
    return float((vol * S.c.array()[species].reshape(len(vol), -1).mean(axis=1)).sum())      # P1: the cell mean is the nodal mean


BALANCE_K_UP = 1500.0        # 1 / s: k dt = 0.15; the cells of tag 1 (c_K = 124 mM against c0 = 4) lose about a seventh of their K per step


def test_global_balance_of_the_injected_species(hip_lib):
    """Three steps with a K source on (0, 1) and three without.  Membrane exchange is internal and the outer boundary carries no flux,
    so the whole-domain integral of c_K differs between the runs by dt * sum over the steps and entries of the row (the basis
    functions sum to one).  The source-free run's own drift of the integral measures what the solves contribute; the bound is ten
    times that plus 1e-6 of the injected amount.  The rate is chosen so that the injected amount is more than a hundred times the
    bound (asserted): a right-hand side that ignored the row, took it on the ECS only, or with another sign or factor, fails."""
    from idealized_common import Constant
    from knpemidg import FieldExpression
    out = {}
    for which in ("free", "source"):
        src = {0: FieldExpression("-k_up * (c_K - c0)", fields=("c_K",), subdomains=(0, 1), k_up=BALANCE_K_UP, c0=4.0)} if which == "source" else {}
        S = _solver(src)
        try:
            t = Constant(0.0)
            tags = np.asarray(S.subdomains.array())
            I, injected, inside = [_integral(S, 0)], 0.0, 0.0
            for k in range(3):
                S.step_membrane_models(k); S.solve_for_time_step(k, t)
                I.append(_integral(S, 0))
                if src:
                    row = S.dev.source_download()[0]
                    injected += float(S.dt) * float(row.sum())
                    inside += float(S.dt) * float(row[tags == 1].sum())
            assert np.isfinite(S.c.array()).all()
            out[which] = (I, injected, inside)
        finally:
            S.dev.close()
    (If, _, _), (Is, injected, inside) = out["free"], out["source"]
    drift = max(abs(i - If[0]) for i in If[1:])
    moved = (Is[-1] - Is[0]) - (If[-1] - If[0])
    bound = 10.0 * drift + 1e-6 * abs(injected)
    print("integral of c_K: %.9e; source-free drift over 3 steps %.3e; injected %.9e (on tag 1: %.9e), moved %.9e, difference %.3e "
          "(bound %.3e, injected / bound %.1f)" % (If[0], drift, injected, inside, moved, abs(moved - injected), bound, abs(injected) / bound))
    assert abs(injected) > 100.0 * bound and abs(inside) > 0.9 * abs(injected)      # the signal is far above the bound, and it sits on tag 1
    assert abs(moved - injected) <= bound


# --------------------------------------------------------------------------------------------------------- 7. a partition's rank
def test_rank_of_a_partition_owned_and_ghost_cells(hip_lib):
    """Rank 0 of a two-slab partition built in one process without a communicator: the row is rank-local, the twin's on the local
    mesh with the local fields, on owned and ghost cells alike."""
    from knpemidg.partition import Partition
    m, s, f = SC.mesh_of("small_3d_844")
    loc = Partition(m, 2, method="slab").local(0)
    sub_l, surf_l = loc.localize(s, f, (1,))
    pb = ko.build_idealized(loc.mesh, sub_l.array(), surf_l.array(), membrane_tags=(1,))
    dev = device_for(pb, nc_owned=loc.nc_owned)
    try:
        tags = np.asarray(sub_l.array())
        U = FC.fields(loc.mesh.num_cells(), dev.nd)
        FC.upload(dev, U)
        case = FC.ALL_FIELDS
        expr = case.expression(FC.T_IN, subdomains=(0, 1))
        dev.source_register(0, expr, ion_names=FC.IONS)
        got = _eval(dev, 0, expr)
        row = _check(got[0], *FC.twin_row(loc.mesh, tags, 1, case, U, FC.T_IN, (0, 1)), "partition rank 0")
        ghost = np.arange(loc.mesh.num_cells()) >= loc.nc_owned
        assert ghost.any() and np.abs(row[ghost]).max() > 0 and np.abs(row[~ghost]).max() > 0
        _check(got[0][~ghost], row[~ghost], FC.twin_row(loc.mesh, tags, 1, case, U, FC.T_IN, (0, 1))[1][~ghost], "owned cells")
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------- 8. resume
def _resume_solver(t):
    # clearance with the window open for 1.5e-4 <= t <= 3.5e-4: steps 2 and 3 (t = 2e-4, 3e-4), the ones behind the checkpoint
    from knpemidg import FieldExpression
    f = FieldExpression("-k_up * (c_K - c0) * ((t0 <= t && t <= t1) ? 1.0 : 0.0)", fields=("c_K",), subdomains=(0, 1), k_up=FC.K_UP, c0=FC.C0,
                        t0=1.5e-4, t1=3.5e-4, t=t)
    return _solver({0: f}, emi_dg_chebyshev=True)


def _steps(S, t, k0, k1):
    snaps = []
    for k in range(k0, k1):
        S.step_membrane_models(k)
        S.solve_for_time_step(k, t)
        snaps.append({"c": S.c.array().copy(), "c_elim": S.ion_list[-1]['c'].array().copy(), "phi": S.phi.array().copy(),
                      "src": np.abs(S.dev.source_download()[0]).max()})
    return snaps


def test_resume_with_a_field_source(hip_lib, tmp_path, monkeypatch):
    """2 steps, checkpoint, a new solver resumed for 2 more with the source on in steps 2 and 3, against 4 steps straight, with the
    yardstick of tests/test_gpu_source.py::test_resume_with_an_expression_source: two uninterrupted runs measure it; bit for bit if
    they agree bit for bit, else within four times their difference.  No new state is checkpointed: the row is recomputed before
    every KNP solve from t and the restored level-n concentrations."""
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


# --------------------------------------------------------------------------------------------------------- 9. refusals, clear, two contexts
def test_abi_refusals_clear_and_close(hip_lib):
    from knpemidg import _abi as A
    mesh, sub, surf = SC.mesh_of("small_3d")
    expr = FC.NONLINEAR.expression(FC.T_IN)
    kernel, code = expr.compiled(3, 4)
    n = len(expr.names)
    i32 = lambda v: np.array(v, dtype=np.int32)

    def raw(dev, species=0, n_params=n, ids=(2, 0), tags=(0,), n_fields=None, n_tags=None):
        ids, tags = i32(ids), i32(tags)
        rc = dev.lib.knp_source_register_fields(dev.ctx, species, code, len(code), kernel.encode(), n_params,
                                                len(ids) if n_fields is None else n_fields, A._p(ids, A._i32p),
                                                len(tags) if n_tags is None else n_tags, A._p(tags, A._i32p))
        return rc, dev.lib.knp_last_error(dev.ctx).decode()
    pb = ko.build_idealized(mesh, sub.array(), surf.array(), membrane_tags=(1,))
    dev = device_for(pb)
    try:
        rc, why = raw(dev)
        assert rc == -1 and "quadrature rule" in why                   # nothing registered yet: no rule
        U = FC.fields(mesh.num_cells(), dev.nd)
        FC.upload(dev, U)
        dev.source_register(0, expr, ion_names=FC.IONS)                # rule and buffer exist from here on
        for species in (-1, dev.n_sys):
            rc, why = raw(dev, species=species)
            assert rc == -1 and "species" in why
        rc, why = raw(dev, n_params=33)
        assert rc == -1 and "parameters" in why
        for ids in ((-1, 0), (2, dev.n_ions + 1)):
            rc, why = raw(dev, ids=ids)
            assert rc == -1 and "field id outside [0, n_ions]" in why
        rc, why = raw(dev, ids=(2, 0, 2))
        assert rc == -1 and "listed twice" in why
        rc, why = raw(dev, ids=tuple(range(4)), n_fields=10)
        assert rc == -1 and "0..9 fields" in why
        for n_tags in (0, -1):
            rc, why = raw(dev, n_tags=n_tags)
            assert rc == -1 and "at least one subdomain tag" in why
        assert raw(dev, ids=(2, dev.n_ions))[0] == 0                   # the eliminated ion's id is n_ions
        assert raw(dev, species=1)[0] == 0
        with pytest.raises(A.KnpError, match="parameter count"):
            dev.source_eval(1, expr.values()[:-1])
        dev.source_register(0, expr, ion_names=FC.IONS)
        assert np.abs(_eval(dev, 0, expr)[0]).max() > 0
        dev.source_clear(0)
        assert np.all(dev.source_download()[0] == 0.0) and 0 not in dev._source_kernels
        with pytest.raises(A.KnpError, match="no source registered"):
            dev.source_eval(0, expr.values())
        dev.source_clear(1)
        dev.set_source(None)                                           # no device source left: the buffer is freed, as before
        assert dev.source_download() is None
        # manufactured-solution mode owns the buffer
        nc, nd = mesh.num_cells(), dev.nd
        dev.set_mms(np.zeros((2, nc)), np.zeros((nc, nd)), np.zeros((2, nc, nd)))
        pb.splitting = 2
        set_params_of(dev, pb)
        rc, why = raw(dev)
        assert rc == -1 and "manufactured" in why
    finally:
        dev.close()


def test_two_contexts_share_nothing(hip_lib):
    """Two contexts built, run and closed interleaved: another mesh, basis, source, subdomains and fields each; closing the first
    leaves the second's rows and kernel in place."""
    a, mesh_a, tags_a, Ua = _device("small_3d", 1)
    b, mesh_b, tags_b, Ub = _device("mesh_2d", 2)
    try:
        ea, eb = FC.NONLINEAR.expression(FC.T_IN, subdomains=(1,)), FC.ALL_FIELDS.expression(FC.T_IN, subdomains=(0, 1))
        a.source_register(0, ea, ion_names=FC.IONS)
        b.source_register(1, eb, ion_names=FC.IONS)
        a.source_eval(0, ea.values()); b.source_eval(1, eb.values())
        ref_b = FC.twin_row(mesh_b, tags_b, 2, FC.ALL_FIELDS, Ub, FC.T_IN, (0, 1))
        _check(a.source_download()[0], *FC.twin_row(mesh_a, tags_a, 1, FC.NONLINEAR, Ua, FC.T_IN, (1,)), "context a")
        first = b.source_download()[1].copy()
        _check(first, *ref_b, "context b")
        a.close()
        assert _eval(b, 1, eb)[1].tobytes() == first.tobytes()
    finally:
        a.close(); b.close()


# --------------------------------------------------------------------------------------------------------- 10. the example
def test_uptake_example_injects_and_clears_potassium(hip_lib):
    """examples/idealized_geometries/run_3D_uptake.py on small_3d(), three steps: the injection window opens behind the first step,
    so K in the box rises in the second by more than it moved in the first, Na falls (the pair is neutral), and with the clearance
    on K ends below the run without it."""
    import run_3D_uptake as RU
    ends = {}
    for clearance in (True, False):
        h = RU.main(steps=3, clearance=clearance, mesh_tuple=small_3d(), n_axons=1)
        S = h["solver"]
        try:
            assert np.isfinite(S.c.array()).all() and np.isfinite(S.phi.array()).all()
            assert sorted(S._device_sources) == [0, 1] and not S._callable_sources
            K, Na = np.asarray(h["K_box"]), np.asarray(h["Na_box"])
            print("clearance %s: K in the box %s, Na %s" % (clearance, K, Na))
            dK, dNa = np.diff(K), np.diff(Na)
            assert dK[1] > 0 and dK[1] > abs(dK[0]) and dNa[1] < 0
            ends[clearance] = K[-1]
        finally:
            S.dev.close()
    assert ends[True] < ends[False]
