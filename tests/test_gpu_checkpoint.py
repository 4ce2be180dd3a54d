"""Checkpoint and resume on the device (csrc/state.hip, Solver.save_checkpoint / load_checkpoint / resume=).

The central test is the bit-for-bit resume: a run that is stopped after some steps, thrown away, rebuilt and continued from the file
must produce the bits of the uninterrupted run -- iteration counts, concentrations, potentials, ODE states, recorder series and
activation map.  Any step-to-step state that the snapshot forgets shows there (withholding the KNP history block alone changes the
iteration counts and the concentrations of the first resumed step).  The yardstick is measured in the same test: two uninterrupted
runs must agree bit for bit themselves; where they do not, four times their measured difference bounds the resumed run instead.
"""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from common import relerr, mean_free

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
for _p in (os.path.join(ROOT, "examples", "idealized_geometries"), os.path.join(ROOT, "examples", "emix_simulations"),
           os.path.join(ROOT, "examples", "custom_membrane_model")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

def _record(S):
    """Probes, one membrane set, gating-variable channels and an activation map; a buffer of 3 rows, so that a checkpoint after 4
    steps finds rows on both sides (3 read back, 1 waiting on the device)."""
    from knpemidg import recorder as R
    mem = R.membrane_facets(S.mesh, S.surfaces.array(), S.membrane_tags)
    return S.record(points=S.mesh.cell_midpoints()[[3, 100]], membrane_sets=[mem[:5]], membrane_states=("n", "m", "h"),
                    membrane_map=dict(threshold=-0.074), capacity=3)


def _rtc_hh():
    """mm_hh as a run-time compiled module built by the factory of tests/rtc_models.py (no built-in device id)."""
    import mm_hh_rtc
    import rtc_models
    from knpemidg.models import _hh_core as core
    return rtc_models.make_model("mm_hh_checkpoint", mm_hh_rtc.HIP_RHS, states=sorted(core.STATE_IND, key=core.STATE_IND.get),
                                 params=sorted(core.PARAM_IND, key=core.PARAM_IND.get), s0=core.init_state_values(),
                                 p0=core.init_parameter_values(), rhs=mm_hh_rtc.rhs)


def _make(case="3d", degree=1, record=False, sp_extra=None, ode_models=None, splitting=True, sp_replace=None):
    """A solver with every setup_* call made, ready to step or to load a checkpoint."""
    if case == "emix":
        import emix_common as E
        from emix_sub import emix_submesh
        S = E.make_solver(mesh_tuple=emix_submesh())
        sp = E.solver_parameters(**(sp_extra or {}))
    else:
        from idealized_common import make_solver, solver_parameters
        from common import small_3d
        dim = 2 if case == "2d" else 3
        small = case == "3d_small"                            # the 768-tet one-axon box of tests/common.py
        S = make_solver(dim=dim, resolution=2 if dim == 2 else 0, n_axons=1 if small else 4, degree=degree, ode_models=ode_models,
                        mesh_tuple=small_3d() if small else None)
        sp = solver_parameters(dim, 0, **(sp_extra or {}))._replace(**(sp_replace or {}))
    if record:
        _record(S)
    S._unpack_solver_params(sp)
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = splitting
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    return S


def _step(S, k, t, mode="active"):
    if mode != "passive":
        S.step_membrane_models(k)
    if k == 0 and S.recorder is not None:
        S.recorder.arm(float(t))
    (S.solve_for_time_step_picard if mode == "picard" else S.solve_for_time_step)(k, t)


def _snapshot(S, t, series=True):
    """Everything the issue lists, as host arrays.  series=False leaves the recorder's rows where they are: reading them empties the
    device buffer, and a checkpoint should find rows waiting there."""
    out = {"t": np.asarray([float(t)]), "emi_niter": np.asarray(S.emi_niter), "knp_niter": np.asarray(S.knp_niter).ravel(),
           "c": S.c.array().copy(), "c_elim": S.ion_list[-1]['c'].array().copy(), "phi": S.phi.array().copy(),
           "phi_M": S.phi_M_prev_PDE.array().copy()}
    for i, m in enumerate(S.mem_models):
        out["ode_states_%d" % i] = np.array(m['ode'].states, copy=True)
        out["ode_params_%d" % i] = np.array(m['ode'].parameters, copy=True)
    if S.recorder is not None:
        if series:
            out["rec_t"], out["rec_rows"] = S.recorder.t.copy(), S.recorder.rows.copy()
        for key, v in S.recorder.membrane_map.items():
            out["map_" + key] = np.asarray(v).copy()
    return out


def _run(S, k0, k1, mode="active", t=None, series_at_end=True):
    """Steps k0 .. k1-1 with a snapshot after each; the recorder's series is read after the last step only (or not at all)."""
    from idealized_common import Constant
    t = Constant(0.0) if t is None else t
    snaps = []
    for k in range(k0, k1):
        _step(S, k, t, mode)
        snaps.append(_snapshot(S, t, series=series_at_end and k == k1 - 1))
    return snaps, t


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _maxdiff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    return float(np.max(np.where(both_nan, 0.0, np.abs(a - b)))) if a.size else 0.0


def _blocks(path):
    from knpemidg import checkpoint as ck
    _, table, arrays, _ = ck.read_checkpoint(path)
    return table, arrays


# ------------------------------------------------------------------------------------------------------------------ 1. round trip
@pytest.mark.parametrize("case,degree,record", [("3d", 1, False), ("3d", 2, False), ("2d", 1, False), ("3d", 1, True)])
def test_round_trip_is_byte_identical(hip_lib, tmp_path, case, degree, record):
    """save -> load into a fresh Solver on the same mesh -> save: the two files hold the same state blocks, byte for byte; so does a
    snapshot taken after a refused load (a recorder of another layout), which must leave the context untouched."""
    from knpemidg import _abi
    A = _make(case, degree, record)
    _run(A, 0, 3)
    p1, p2 = str(tmp_path / "a.h5"), str(tmp_path / "b.h5")
    A.save_checkpoint(p1)
    raw = A.dev.state_save()
    B = _make(case, degree, record)
    if not record:
        other = _make(case, degree, True)                       # its snapshot has the recorder's blocks: not this context's list
        before = B.dev.state_save()
        with pytest.raises(_abi.KnpError, match="knp_state_load"):
            B.dev.state_load(other.dev.state_save())
        assert _same_bits(before, B.dev.state_save())
        other.dev.close()
    assert B.load_checkpoint(p1) == 3
    B.save_checkpoint(p2)
    assert _same_bits(raw, B.dev.state_save())
    (t1, a1), (t2, a2) = _blocks(p1), _blocks(p2)
    assert t1.tobytes() == t2.tobytes() and len(a1) >= 13
    for b, x, y in zip(t1, a1, a2):
        assert _same_bits(x, y), int(b["id"])
    # caller numbering: the per-cell block of phi IS what the download path (host permutation) returns
    phi = a1[[int(b["id"]) for b in t1].index(1)]
    assert _same_bits(phi.ravel(), A.phi.array().ravel())
    kinds = {int(b["kind"]) for b in t1}
    assert kinds == {0, 1, 2, 3}
    A.dev.close(); B.dev.close()


# ------------------------------------------------------------------------------------------------------------------ 2. bit-exact resume
@pytest.mark.parametrize("mode,degree,n1,n2", [("active", 1, 4, 4), ("active", 2, 4, 2), ("picard", 1, 2, 2), ("rtc", 1, 4, 4)])
def test_resume_is_bit_exact(hip_lib, tmp_path, monkeypatch, mode, degree, n1, n2):
    """3D r=0, HH with the stimulus on, block-Jacobi preconditioner only (nothing is rebuilt from another kappa), Chebyshev choice
    pinned.  A: n1 + n2 steps straight.  B: n1 steps, checkpoint (history full, stimulus non-zero at t = 4e-4 s), Solver discarded,
    a new one resumed for n2 steps.  Steps n1+1 .. n1+n2 of B must be A's, bit for bit; A' measures the yardstick first."""
    monkeypatch.setenv("KNP_NO_AMG", "1")
    kw = dict(degree=degree, record=True, sp_extra=dict(emi_dg_chebyshev=True))
    case = "3d"
    if mode == "picard":
        # the configuration tests/test_gpu_solver.py drives the Picard variant with (one-axon box, tight Krylov tolerances: the Picard
        # loop stops on a 1e-4 update and exits the process when it does not get there); every Picard level is a solve, so the
        # histories are full after the first step
        case, kw["sp_replace"] = "3d_small", dict(rtol_emi=1e-9, rtol_knp=1e-11)
    step_mode = "active" if mode == "rtc" else mode
    if mode == "rtc":
        from knpemidg.models import mm_hh_no_stim
        kw["ode_models"] = {1: _rtc_hh(), 2: mm_hh_no_stim}
    path = str(tmp_path / "ck.h5")
    runs = []
    for _ in range(2):                                            # A and A'
        S = _make(case, **kw)
        assert not S.use_amg
        runs.append(_run(S, 0, n1 + n2, step_mode)[0])
        S.dev.close()
    A, A2 = runs
    yard = {key: max(_maxdiff(a[key], b[key]) for a, b in zip(A, A2)) for key in A[0]}
    exact = all(_same_bits(a[key], b[key]) for a, b in zip(A, A2) for key in a)
    print("yardstick A vs A' (max-norm per field):", {k: v for k, v in yard.items() if v}, "bit-identical:", exact)
    assert all(_same_bits(a[key], b[key]) for a, b in zip(A, A2) for key in ("emi_niter", "knp_niter"))
    B1 = _make(case, **kw)
    if mode == "rtc":
        assert B1.mem_models[0]['ode'].handle is not None and getattr(B1.mem_models[0]['ode'].ode, "MODEL_ID", None) is None
    _run(B1, 0, n1, step_mode, series_at_end=False)
    assert B1.recorder._waiting == (n1 - 1) % 3 + 1 and len(B1.recorder._rows) == (n1 - 1) // 3      # rows waiting in the device buffer
    B1.save_checkpoint(path)
    B1.dev.close()
    del B1
    B2 = _make(case, **kw)
    from idealized_common import Constant
    t = Constant(0.0)
    assert B2.load_checkpoint(path, t=t, picard=mode == "picard") == n1
    assert float(t) == A[n1 - 1]["t"][0]
    B, _ = _run(B2, n1, n1 + n2, step_mode, t=t)
    B2.dev.close()
    assert len(B) == n2
    for j, b in enumerate(B):
        a = A[n1 + j]
        assert set(b) <= set(a) and (j < n2 - 1 or set(a) == set(b))
        assert _same_bits(a["emi_niter"], b["emi_niter"]) and _same_bits(a["knp_niter"], b["knp_niter"]), (j, a["emi_niter"], b["emi_niter"])
        for key in b:
            if exact:
                assert _same_bits(a[key], b[key]), (mode, "step", n1 + j + 1, key, _maxdiff(a[key], b[key]))
            else:
                assert _maxdiff(a[key], b[key]) <= 4.0 * yard[key], (mode, "step", n1 + j + 1, key, _maxdiff(a[key], b[key]), yard[key])
    # the run really did something at the checkpoint: stimulus on, potential moving, full histories
    assert np.abs(A[n1]["phi_M"] - A[n1 - 1]["phi_M"]).max() > 0 and len(A[-1]["rec_t"]) == n1 + n2
    if mode == "picard":
        assert B2.picard_iters[:n1] and len(B2.picard_iters) == n1 + n2


def _mms_passive(steps, **kw):
    """The passive loop on the configuration the repository runs it with: the time-dependent manufactured solution of
    examples/mms/run_MMS_time.py (its data terms are re-integrated at the caller's t before every step) on a 8 x 8 mesh."""
    from collections import namedtuple
    ex = os.path.join(ROOT, "examples", "mms")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    from knpemidg import Solver, Constant, make_mesh_MMS
    from mms_time import setup_mms
    dt = 2.5e-3
    names = ('D_a1', 'D_a2', 'D_b1', 'D_b2', 'D_c1', 'D_c2', 'C_a1', 'C_a2', 'C_b1', 'C_b2', 'C_c1', 'C_c2', 'C_phi',
             'z_a', 'z_b', 'z_c', 'dt', 'F', 'C_M', 'phi_M_init', 'R', 'temperature', 'phi_M_init_type', 'rho_sub')
    vals = (6, 5, 3, 4, 1, 2, 1, 2, 2, 4, 3, 2, 1.0 / dt, 1.0, -1.0, 1.0, dt, 1.0, 1.0, None, 1.0, 1.0, 'expression', {0: 0.0, 1: 0.0, 2: 0.0})
    params = namedtuple('params', names)(*vals)
    mesh, subdomains, surfaces = make_mesh_MMS(3)
    t = Constant(0.0)
    mms = setup_mms(params, t)
    sol, rhs = mms.solution, mms.rhs

    def ion(s, name):
        return {'D_sub': {1: getattr(params, 'D_%s1' % s), 0: getattr(params, 'D_%s2' % s)}, 'z': getattr(params, 'z_' + s),
                'c_init_sub': {1: sol['c_%s1_init' % s], 0: sol['c_%s2_init' % s]}, 'c_init_sub_type': 'expression',
                'f1': rhs['volume_c_%s1' % s], 'f2': rhs['volume_c_%s2' % s], 'g_robin_1': rhs['bdry']['u_%s1' % s],
                'g_robin_2': rhs['bdry']['u_%s2' % s], 'bdry': rhs['bdry']['neumann_' + s],
                'C_sub': {1: getattr(params, 'C_%s1' % s), 0: getattr(params, 'C_%s2' % s)}, 'name': name, 'f_source': 0.0}
    S = Solver(params=params, ion_list=[ion('a', 'Na'), ion('b', 'K'), ion('c', 'Cl')], degree_emi=1, degree_knp=1, mms=mms)
    S.verbose = False
    S.setup_domain(mesh, subdomains, surfaces)
    S.setup_parameters()
    S.setup_FEM_spaces()
    sp = namedtuple('solver_params', ('direct_emi', 'direct_knp', 'resolution', 'rtol_emi', 'rtol_knp', 'atol_emi', 'atol_knp',
                                      'threshold_emi', 'threshold_knp'))(True, True, 3, 1e-6, 1e-7, 1e-40, 1e-40, 0.9, 7.5)
    S.solve_system_passive(steps * dt, t, sp, None, **kw)
    out = _snapshot(S, t)
    S.dev.close()
    return out


def test_passive_loop_resume_is_bit_exact(hip_lib, tmp_path):
    """solve_system_passive through its own loop: 8 steps straight (twice: the yardstick) against 4 steps with checkpoint_every=4 and a
    second solver resumed from the file for the other 4.  The data of this problem depend on t, which the resume restores into the
    caller's t object; k continues at 4.  Final fields and the per-step iteration counts of all 8 steps must be the same bits."""
    path = str(tmp_path / "passive.h5")
    A, A2 = _mms_passive(8), _mms_passive(8)
    exact = all(_same_bits(A[key], A2[key]) for key in A)
    yard = {key: _maxdiff(A[key], A2[key]) for key in A}
    print("yardstick A vs A' (max-norm per field):", {k: v for k, v in yard.items() if v}, "bit-identical:", exact)
    first = _mms_passive(4, checkpoint_every=4, checkpoint_file=path)
    assert os.path.exists(path) and abs(first["t"][0] - 1.0e-2) < 1e-15
    B = _mms_passive(8, resume=path)
    assert len(B["emi_niter"]) == 8 and _same_bits(A["emi_niter"], B["emi_niter"]) and _same_bits(A["knp_niter"], B["knp_niter"])
    assert not _same_bits(first["c"], B["c"])                                     # the second half moved the state
    for key in A:
        if exact:
            assert _same_bits(A[key], B[key]), (key, _maxdiff(A[key], B[key]))
        else:
            assert _maxdiff(A[key], B[key]) <= 4.0 * yard[key], (key, _maxdiff(A[key], B[key]), yard[key])


# ------------------------------------------------------------------------------------------------------------------ 3 + 4. default preconditioner
def _traj_errors(S, g, k):
    from test_gpu_trajectory import _errors, _cell_volumes
    return _errors(S, g, k, _cell_volumes(S.mesh))


def _pair_errors(a, b, vol):
    nz = np.nonzero(b["phi_M"])[0]
    return dict(c=relerr(a["c"], b["c"]), c_elim=relerr(a["c_elim"], b["c_elim"]),
                phi=relerr(mean_free(a["phi"], vol), mean_free(b["phi"], vol)), phi_M=relerr(a["phi_M"][nz], b["phi_M"][nz]))


@pytest.mark.parametrize("case,gold", [("3d", "traj_3D_r0_4axon_P1"), ("emix", "traj_emix_sub_P1")])
def test_resume_with_default_preconditioner(hip_lib, tmp_path, case, gold):
    """AMG on, smoother as the first part measured it.  The hierarchy after the resume is built from the restored kappa, so iterates
    differ within the stopping tolerances: A and B agree to the bounds tests/test_gpu_trajectory.py holds the same case to against its
    golden trajectory (c, c_elim 1e-6; mean-free phi, phi_M 1e-4), both meet them against the golden file, and the iteration counts
    differ by at most 1 per step (the margin of tests/test_gpu_multirank.py).  The first resumed step makes ONE EMI solve -- no
    smoother trial -- with the recorded smoother."""
    from test_gpu_trajectory import _cell_volumes
    from knpemidg import checkpoint as ck
    from idealized_common import Constant
    g = np.load(os.path.join(GOLD, gold + ".npz"))
    path = str(tmp_path / "ck.h5")
    n1 = n2 = 4
    B1 = _make(case)
    assert B1.use_amg and B1._emi_trial is True
    _run(B1, 0, n1)
    chosen = B1._emi_cheb_chosen
    trial_ran = B1._emi_trial is None              # the first step measured both smoothers and kept one
    assert trial_ran and chosen == B1.emi_dg_chebyshev_measured["chosen"]
    B1.save_checkpoint(path)
    header = ck.read_checkpoint(path)[0]
    assert header["emi_dg_chebyshev"] == chosen and header["k"] == n1 and header["amg_refresh"]["solves"] == n1
    assert header["emi_trial_pending"] == (not trial_ran)
    B1.dev.close()
    A = _make(case, sp_extra=dict(emi_dg_chebyshev=chosen))      # the straight run with the same smoother
    vol = _cell_volumes(A.mesh)
    t = Constant(0.0)
    ref = []
    for k in range(n1 + n2):
        _step(A, k, t)
        ref.append(_snapshot(A, t))
        e = _traj_errors(A, g, k)
        assert e["c"] < 1e-6 and e["c_elim"] < 1e-6 and e["phi"] < 1e-4 and e["phi_M"] < 1e-4, ("A", k, e)
    A.dev.close()
    B2 = _make(case)
    solves = []
    real = B2.dev.emi_solve
    B2.dev.emi_solve = lambda *a, **k: (solves.append(1), real(*a, **k))[1]
    tb = Constant(0.0)
    assert B2.load_checkpoint(path, t=tb) == n1 and (B2._emi_trial is None) == trial_ran and B2._emi_cheb_chosen == chosen
    for k in range(n1, n1 + n2):
        _step(B2, k, tb)
        if k == n1:
            assert len(solves) == 1, solves
        b = _snapshot(B2, tb)
        e = _traj_errors(B2, g, k)
        assert e["c"] < 1e-6 and e["c_elim"] < 1e-6 and e["phi"] < 1e-4 and e["phi_M"] < 1e-4, ("B", k, e)
        d = _pair_errors(b, ref[k], vol)
        assert d["c"] < 1e-6 and d["c_elim"] < 1e-6 and d["phi"] < 1e-4 and d["phi_M"] < 1e-4, (k, d)
        assert abs(int(b["emi_niter"][-1]) - int(ref[k]["emi_niter"][-1])) <= 1, (k, b["emi_niter"], ref[k]["emi_niter"])
        assert np.abs(b["knp_niter"][-B2.N_ions:] - ref[k]["knp_niter"][-B2.N_ions:]).max() <= 1, (k, b["knp_niter"], ref[k]["knp_niter"])
    assert len(solves) == n2
    B2.dev.close()


# ------------------------------------------------------------------------------------------------------------------ 5. ordering
def test_checkpoint_is_independent_of_device_ordering_and_kernel_family(hip_lib, tmp_path, monkeypatch):
    """Written by a context with the Morton cell order and the halo-staged P1 applies, loaded by one that keeps the caller's order
    (KNP_NO_REORDER=1) and runs another apply family (KNP_APPLY_HALO=0, KNP_EMI_RING=0): the per-cell blocks are in the caller's numbering, so the next
    steps agree with the straight run to the bounds of the trajectory tests (the summation orders differ: not bit for bit)."""
    from test_gpu_trajectory import _cell_volumes
    from idealized_common import Constant
    monkeypatch.setenv("KNP_NO_AMG", "1")
    path = str(tmp_path / "ck.h5")
    A = _make("3d", sp_extra=dict(emi_dg_chebyshev=True))
    assert not np.array_equal(A.dev.cell_order, np.arange(A.dev.nc))
    variant_a = (A.dev.apply_variant(0), A.dev.apply_variant(1))
    ref, _ = _run(A, 0, 6)
    vol = _cell_volumes(A.mesh)
    A.dev.close()
    B1 = _make("3d", sp_extra=dict(emi_dg_chebyshev=True))
    _run(B1, 0, 4)
    B1.save_checkpoint(path)
    B1.dev.close()
    monkeypatch.setenv("KNP_NO_REORDER", "1")
    monkeypatch.setenv("KNP_APPLY_HALO", "0")
    monkeypatch.setenv("KNP_EMI_RING", "0")
    B2 = _make("3d", sp_extra=dict(emi_dg_chebyshev=True))
    assert np.array_equal(B2.dev.cell_order, np.arange(B2.dev.nc))
    assert (B2.dev.apply_variant(0), B2.dev.apply_variant(1)) != variant_a
    t = Constant(0.0)
    assert B2.load_checkpoint(path, t=t) == 4
    assert _same_bits(B2.c.array(), ref[3]["c"]) and _same_bits(B2.phi.array(), ref[3]["phi"])     # the restored state itself: exact
    got, _ = _run(B2, 4, 6, t=t)
    for j, b in enumerate(got):
        d = _pair_errors(b, ref[4 + j], vol)
        assert d["c"] < 1e-6 and d["c_elim"] < 1e-6 and d["phi"] < 1e-4 and d["phi_M"] < 1e-4, (j, d)
        assert np.abs(b["emi_niter"][-1] - ref[4 + j]["emi_niter"][-1]) <= 1
    B2.dev.close()


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refused_loads_leave_the_solver_working(hip_lib, tmp_path, monkeypatch):
    """A P1 checkpoint does not load into a P2 solver, one of another mesh not into this one, one without a recorder not into a
    solver with one: KnpError naming what differs, and the refusing solver then takes its first step like a solver that was never
    asked (compared with a fresh one of the same configuration)."""
    from knpemidg import _abi
    monkeypatch.setenv("KNP_NO_AMG", "1")
    path = str(tmp_path / "p1.h5")
    W = _make("3d")
    _run(W, 0, 2)
    W.save_checkpoint(path)
    W.dev.close()
    for what, kw, match in (("degree", dict(case="3d", degree=2), "field 'degrees'"), ("mesh", dict(case="3d_small"), "field 'mesh_hash'"),
                            ("recorder", dict(case="3d", record=True), "state blocks in the file")):
        S = _make(**kw)
        with pytest.raises(_abi.KnpError, match=match):
            S.load_checkpoint(path)
        got, _ = _run(S, 0, 1)
        S.dev.close()
        F = _make(**kw)
        want, _ = _run(F, 0, 1)
        F.dev.close()
        for key in ("c", "c_elim", "phi", "phi_M", "emi_niter", "knp_niter"):
            assert _same_bits(got[0][key], want[0][key]) or relerr(got[0][key], want[0][key]) < 1e-12, (what, key)


def test_several_ranks_are_refused_without_hanging(hip_lib, tmp_path):
    """Two ranks on one GPU (shared-memory communicator): save_checkpoint, the C entry point and load_checkpoint each raise the
    'several ranks' error; no rank enters a collective, so nothing waits."""
    name = "/knp_%s" % uuid.uuid4().hex[:16]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "checkpoint_rank_worker.py"), str(r), "2", name, str(tmp_path)],
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
    assert all(l.count("several ranks") >= 3 for l in logs), logs


# ------------------------------------------------------------------------------------------------------------------ 7. off means off
def test_defaults_write_nothing_and_saving_does_not_perturb(hip_lib, tmp_path, monkeypatch):
    """solve_system_active with the three new arguments at their defaults creates no file; with checkpoint_every=2 the state after 4
    steps is the same bits.  The file of step 4 then resumes through solve_system_active(resume=...) to the bits of a straight
    6-step run (solve_system_passive: test_passive_loop_resume_is_bit_exact)."""
    from idealized_common import make_solver, solver_parameters, Constant
    monkeypatch.setenv("KNP_NO_AMG", "1")
    sp = solver_parameters(3, 0, emi_dg_chebyshev=True)

    def run(active, steps, folder, **kw):
        S = make_solver(dim=3, resolution=0, n_axons=4)
        _record(S)
        os.makedirs(folder, exist_ok=True)
        t = Constant(0.0)
        if active:
            S.solve_system_active(steps * 1e-4, t, sp, filename=folder + "/", **kw)
        else:
            S.solve_system_passive(steps * 1e-4, t, sp, None, filename=folder + "/", **kw)
        out = _snapshot(S, t)
        S.dev.close()
        return out

    for active in (True,):
        d = str(tmp_path / ("active" if active else "passive"))
        plain = run(active, 4, d + "/plain")
        assert sorted(os.listdir(d + "/plain")) == ["timeseries.h5"]                  # what an existing call writes, nothing new
        saved = run(active, 4, d + "/saved", checkpoint_every=2)
        assert sorted(os.listdir(d + "/saved")) == ["checkpoint.h5", "timeseries.h5"]
        for key in plain:
            assert _same_bits(plain[key], saved[key]), (active, key)
        straight = run(active, 6, d + "/straight")
        resumed = run(active, 6, d + "/resumed", resume=d + "/saved/checkpoint.h5", checkpoint_file=d + "/resumed/other.h5")
        assert "other.h5" not in os.listdir(d + "/resumed")                           # checkpoint_every stayed off
        for key in straight:
            assert _same_bits(straight[key], resumed[key]), (active, key, _maxdiff(straight[key], resumed[key]))
        assert len(resumed["rec_t"]) == 6                                             # the uninterrupted series
