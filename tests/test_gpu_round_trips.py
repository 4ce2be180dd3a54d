"""Fewer host round trips per time step, none of which may change a bit: the solves' epilogues read the last
look's host copy (KNP_FOLD_EPILOGUE), no look before the first iteration when the previous solve iterated (KNP_POLL_FIRST),
knp_sync in one trip (KNP_SYNC_ONE_TRIP).  Each against its old path on three stimulated steps of the 4-axon mesh with
its AMG hierarchies (PCG for EMI; BiCGStab and GMRES for KNP), all three together, the converged-at-entry solve behind a skipped
look and the count of blocking waits per step."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "idealized_geometries"))

# switch -> the value that restores the old path
OLD = {"KNP_FOLD_EPILOGUE": "0", "KNP_POLL_FIRST": "1", "KNP_SYNC_ONE_TRIP": "0"}
KRYLOV = ("bicgstab", "gmres")
_runs = {}          # (krylov, names of the switches set to old) -> result of _three_steps: computed once, shared, never changed


def _make_solver(krylov):
    from idealized_common import make_solver, solver_parameters
    S = make_solver(dim=3, resolution=0, n_axons=4)
    S._unpack_solver_params(solver_parameters(3, 0))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    S.dev.set_knp_krylov(krylov)
    assert S.use_amg
    return S


def _three_steps(krylov):
    from idealized_common import Constant
    from knpemidg import _abi as A
    S = _make_solver(krylov)
    dev = S.dev
    triples = []                                   # every solve's returned residual triple(s), in call order
    emi_solve, knp_solve = dev.emi_solve, dev.knp_solve

    def rec_emi(*a, **k):
        n, r = emi_solve(*a, **k)
        triples.append(np.array(r, dtype=np.float64).ravel().copy())
        return n, r

    def rec_knp(*a, **k):
        n, r = knp_solve(*a, **k)
        triples.append(np.array(r, dtype=np.float64).ravel().copy())
        return n, r

    dev.emi_solve, dev.knp_solve = rec_emi, rec_knp
    t = Constant(0.0)
    trips = []
    for k in range(3):
        S.step_membrane_models(k)
        S.solve_for_time_step(k, t)
        trips.append(dev.host_round_trips())
    out = {"phi": S.phi.array().copy(), "c": S.c.array().copy(), "c_elim": dev.download(A.F_C_ELIM).copy(),
           "phi_M": S.phi_M_prev_PDE.array().copy(), "emi_niter": list(S.emi_niter), "knp_niter": [list(n) for n in S.knp_niter],
           "triples": np.concatenate(triples), "trips_steps_2_3": trips[2] - trips[0]}
    dev.close()
    return out


def _run(monkeypatch, krylov, old_switches):
    key = (krylov, tuple(sorted(old_switches)))
    if key not in _runs:
        for name in OLD:
            monkeypatch.delenv(name, raising=False)
        for name in old_switches:
            monkeypatch.setenv(name, OLD[name])
        _runs[key] = _three_steps(krylov)
        for name in old_switches:
            monkeypatch.delenv(name, raising=False)
    return _runs[key]


def _assert_bitwise(a, b, what):
    assert a["emi_niter"] == b["emi_niter"] and a["knp_niter"] == b["knp_niter"], (what, a["emi_niter"], b["emi_niter"], a["knp_niter"], b["knp_niter"])
    for name in ("phi", "c", "c_elim", "phi_M", "triples"):
        assert np.array_equal(a[name], b[name]), (what, name)


@pytest.mark.parametrize("old", list(OLD) + ["all"])
def test_round_trip_switches_are_bitwise(hip_lib, monkeypatch, old):
    """Three stimulated steps with the new paths against the same steps with one switch (or all of them) on its old path."""
    monkeypatch.setenv("KNP_AMG_MAXCOARSE", "300")
    switches = list(OLD) if old == "all" else [old]
    for krylov in KRYLOV:
        new = _run(monkeypatch, krylov, [])
        assert min(new["emi_niter"]) >= 1 and min(min(n) for n in new["knp_niter"]) >= 1      # predictions exist from step 2 on
        _assert_bitwise(new, _run(monkeypatch, krylov, switches), (krylov, old))


def test_round_trips_per_step(hip_lib, monkeypatch):
    """Blocking waits of steps 2 and 3 (predictions exist), new paths against all old ones in the same process: at least
    6 fewer per step -- 2 first looks, 2 epilogue copies, 2 second trips of knp_sync.

    Measured on MI355X, 4-axon r=0 mesh, steps 2 + 3 together: 10 with the new paths, 22 with all old ones, for BiCGStab and for
    GMRES alike -- 5 against 11 per step (not asserted)."""
    monkeypatch.setenv("KNP_AMG_MAXCOARSE", "300")
    for krylov in KRYLOV:
        new = _run(monkeypatch, krylov, [])["trips_steps_2_3"]
        old = _run(monkeypatch, krylov, list(OLD))["trips_steps_2_3"]
        print("host round trips of steps 2 + 3, %s: new %d, all old %d" % (krylov, new, old))
        assert old - new >= 2 * 6, (krylov, new, old)


def test_converged_at_entry_behind_a_skipped_look(hip_lib, monkeypatch):
    """A system whose init reduction sets the status word while the look behind it is skipped (a prediction >= 1 exists and a state
    upload keeps it): the chunk of launches enqueued blind must change nothing.  EMI with PETSc's test (residual target 0) and KNP
    with GMRES and min_it = 0: the second solve from the uploaded solution returns 0 iterations and leaves the field bitwise alone,
    with the look skipped and (KNP_POLL_FIRST=1) with the look taken.  BiCGStab tests no tolerance at entry (only an exactly zero
    residual ends it there), so its solve from the uploaded solution takes one iteration: that one is compared bitwise between the
    skipped and the taken look."""
    from idealized_common import Constant
    from knpemidg import _abi as A
    monkeypatch.setenv("KNP_AMG_MAXCOARSE", "300")
    for name in OLD:
        monkeypatch.delenv(name, raising=False)
    for krylov in KRYLOV:
        S = _make_solver(krylov)
        dev = S.dev
        try:
            t = Constant(0.0)
            S.step_membrane_models(0)
            S.solve_for_time_step(0, t)             # hierarchies, lagged inverses and both predictions exist behind this step
            assert S.emi_niter[0] >= 1 and min(S.knp_niter[0]) >= 1
            # EMI
            dev.emi_residual_target(0.0)
            dev.update_kappa(); dev.emi_rhs()
            n1, _ = dev.emi_solve(1e-8, 1e-40, maxit=200)
            assert n1 >= 1
            phi = dev.download(A.F_PHI).copy()
            for first in (None, "1"):
                if first is None:
                    monkeypatch.delenv("KNP_POLL_FIRST", raising=False)
                else:
                    monkeypatch.setenv("KNP_POLL_FIRST", first)
                dev.upload(A.F_PHI, phi)
                n2, r2 = dev.emi_solve(1e-3, 1e-40, maxit=200)
                assert n2 == 0, (krylov, first, n2, r2)
                assert np.array_equal(dev.download(A.F_PHI), phi), (krylov, first)
            monkeypatch.delenv("KNP_POLL_FIRST", raising=False)
            # KNP
            dev.update_dnphi(); dev.knp_rhs()
            n1, _ = dev.knp_solve(1e-12, 1e-40, maxit=200, min_it=0)
            assert min(n1) >= 1
            c = dev.download(A.F_C).copy()
            got = {}
            for first in (None, "1"):
                if first is None:
                    monkeypatch.delenv("KNP_POLL_FIRST", raising=False)
                else:
                    monkeypatch.setenv("KNP_POLL_FIRST", first)
                dev.upload(A.F_C, c)
                n2, r2 = dev.knp_solve(1e-4, 1e-40, maxit=200, min_it=0)
                got[first] = (list(n2), np.array(r2).copy(), dev.download(A.F_C).copy())
                if krylov == "gmres":
                    assert max(n2) == 0, (first, n2, r2)
                    assert np.array_equal(got[first][2], c), first
                else:
                    assert max(n2) <= 1, (first, n2, r2)
            monkeypatch.delenv("KNP_POLL_FIRST", raising=False)
            assert got[None][0] == got["1"][0] and np.array_equal(got[None][1], got["1"][1]) and np.array_equal(got[None][2], got["1"][2]), krylov
        finally:
            dev.close()

