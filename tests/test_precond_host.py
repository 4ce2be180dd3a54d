"""CPU tests of the preconditioner's host side (knpemidg/precond.py: the measured smoother choice, the refresh policy of the lagged EMI
hierarchy and its checkpoint entry) and of the effective solver settings (knpemidg/solver.py: resolve_settings), each against a stand-in
device: no GPU, no library."""
from collections import namedtuple

import numpy as np
import pytest

from knpemidg import _abi
from knpemidg.precond import AmgInputs, AmgSetup, SmootherChoice
from knpemidg.solver import EMI_TARGET_SAFETY, PHI_ENERGY_FACTOR, resolve_settings


# ---- the EMI DG-level smoother -----------------------------------------------------------------------------------------------------
class TrialDev:
    def __init__(self):
        self.calls, self.reduced, self.uploads = [], [], 0

    def set_emi_dg_smoother(self, on):
        self.calls.append(bool(on))

    def allreduce_sum(self, v):
        self.reduced.append(list(v))
        return np.asarray(v, dtype=float) * 3.0          # three ranks with the same timings

    def download(self, field):
        return np.zeros(4)

    def upload(self, field, a):
        self.uploads += 1


def _trial(cost_on, cost_off, explicit=None, recorded=None):
    dev = TrialDev()
    C = SmootherChoice(dev, setting=explicit, recorded=recorded, verbose=False)
    first = C.chosen
    assert C.measured is None
    if not C.pending:
        return first, dev.calls, None, None

    def solve():                                         # one decade of reduction: seconds = cost per decade
        on = dev.calls[-1]
        return (cost_on if on else cost_off), (7 if on else 9), [1.0, 0.1, 0.0]
    out = C.run_trial(solve)
    assert C.pending is False and len(dev.reduced) == 1 and C.chosen == C.measured["chosen"]
    return first, dev.calls, C.measured, out


def test_emi_dg_smoother_is_chosen_by_measurement(monkeypatch):
    """precond.SmootherChoice -- round 3 read the DG-level smoother of the EMI preconditioner off mesh-size thresholds; round 4 measures
    it on the first EMI system of the run: the same system is solved from the same initial guess with and without the Chebyshev step
    (one untimed solve each first), each charged its time per decade of true-residual reduction, the costs all-reduced (every rank of a
    partitioned run takes the same decision), the step dropped only if that is >= 3 % cheaper; the step's solution comes from a solve
    with the chosen variant; solver_params / KNP_EMI_CHEB decide explicitly, and so does the choice a checkpoint recorded."""
    monkeypatch.delenv("KNP_EMI_CHEB", raising=False)
    first, calls, m, out = _trial(1.0, 0.8)                   # plain block-Jacobi 20 % cheaper per decade: dropped
    assert first is True and calls == [True, False, True, False] and m["chosen"] is False and out[1] == 9
    first, calls, m, out = _trial(1.0, 0.99)                  # within the 3 % margin: the step stays, the step's solve is redone with it
    assert calls == [True, False, True, False, True] and m["chosen"] is True and out[1] == 7
    first, calls, m, out = _trial(1.0, 1.25)
    assert calls[-1] is True and abs(m["plain_s_per_decade"] - 3.0 * 1.25) < 1e-12
    assert _trial(None, None, explicit=False)[0] is False and _trial(None, None, explicit=True)[0] is True      # explicit: no trial
    for recorded in (False, True, 0, 1):                      # a resume header's value: no trial, and that smoother
        first, calls, m, out = _trial(None, None, recorded=recorded)
        assert first is bool(recorded) and calls == [] and m is None and out is None
    assert _trial(None, None, explicit=True, recorded=False)[0] is True           # an explicit setting overrides the recorded value
    assert _trial(None, None, explicit=False, recorded=True)[0] is False
    monkeypatch.setenv("KNP_EMI_CHEB", "0")
    assert _trial(None, None)[0] is False
    assert _trial(None, None, recorded=True)[0] is False
    assert _trial(None, None, explicit=True)[0] is True       # the field beats the variable


def test_a_loaded_checkpoint_sets_the_recorded_smoother(monkeypatch):
    """SmootherChoice.resume (Solver.load_checkpoint): the recorded smoother goes to the device and the trial is off, unless
    solver_params decide."""
    monkeypatch.delenv("KNP_EMI_CHEB", raising=False)
    for setting, recorded, want in ((None, False, False), (None, 1, True), (True, False, True), (False, True, False)):
        dev = TrialDev()
        C = SmootherChoice(dev, setting=setting, verbose=False)
        assert C.pending is (setting is None)
        C.resume(recorded)
        assert C.chosen is want and C.pending is False and dev.calls == [want] and C.measured is None


# ---- the refresh policy of the lagged EMI hierarchy ----------------------------------------------------------------------------------
class KappaDev:
    """download(F_KAPPA) returns what the test scripted"""
    def __init__(self, kappa):
        self.kappa = np.asarray(kappa, dtype=np.float64)

    def download(self, field):
        assert field == _abi.F_KAPPA
        return self.kappa.copy()


def _setup(kappa0, local_mesh=None):
    A = AmgSetup(AmgInputs(*[None] * len(AmgInputs._fields))._replace(local_mesh=local_mesh, verbose=False))
    A.kappa0 = np.asarray(kappa0, dtype=np.float64)
    A.rebuilds = []

    def rebuild(dev):                                        # stands in for setup_emi: a new hierarchy from the current kappa
        A.rebuilds.append(A.refresh["solves"])
        A.kappa0 = dev.kappa.copy()
    A.setup_emi = rebuild
    return A


def _solves(A, dev, counts, history=None):
    history = [] if history is None else history
    for n in counts:
        history.append(n)
        A.maybe_refresh_emi(dev, history)
    return history


def test_kappa_drift_rebuilds_the_hierarchy_at_the_check(monkeypatch):
    monkeypatch.delenv("KNP_AMG_REFRESH_EVERY", raising=False)
    monkeypatch.delenv("KNP_AMG_REFRESH_KAPPA", raising=False)
    k0 = np.array([1.0, 2.0, 4.0])
    A, dev = _setup(k0), KappaDev(3.0 * k0)
    h = _solves(A, dev, [5] * 49)
    assert A.rebuilds == [] and A.refreshes == 0 and A.refresh["solves"] == 49       # kappa is looked at every 50th solve only
    _solves(A, dev, [5], h)
    assert A.rebuilds == [50] and A.refreshes == 1
    assert A.refresh == {"solves": 0, "ref": None, "high": 0}                        # the counters start over
    assert np.array_equal(A.kappa0, 3.0 * k0)
    _solves(A, dev, [5] * 50, h)
    assert A.refreshes == 1                                                          # built from this kappa: no drift
    monkeypatch.setenv("KNP_AMG_REFRESH_EVERY", "4")                                 # read at every solve
    A, dev = _setup(k0), KappaDev(k0 * [1.0, 1.25, 0.75])
    _solves(A, dev, [5] * 8)
    assert A.rebuilds == []                                                          # 25 % is the limit, not beyond it
    dev.kappa[2] = 4.0 * 0.74
    _solves(A, dev, [5] * 3)
    assert A.rebuilds == []
    _solves(A, dev, [5])
    assert A.rebuilds == [12] and A.refresh["solves"] == 0
    monkeypatch.setenv("KNP_AMG_REFRESH_KAPPA", "0.5")
    A, dev = _setup(k0), KappaDev(1.4 * k0)
    _solves(A, dev, [5] * 4)
    assert A.rebuilds == []
    dev.kappa[0] = 1.51
    _solves(A, dev, [5] * 4)
    assert A.rebuilds == [8]


def test_zero_and_non_finite_kappa(monkeypatch):
    monkeypatch.setenv("KNP_AMG_REFRESH_EVERY", "1")
    monkeypatch.delenv("KNP_AMG_REFRESH_KAPPA", raising=False)
    k0 = np.array([0.0, 1.0, 2.0])
    A, dev = _setup(k0), KappaDev([0.0, 1.0, 2.0])
    _solves(A, dev, [5, 5])
    dev.kappa[0] = 4.0e-13                      # against the floor 1e-12 max|kappa0| = 2e-12 this is a drift of 0.2, not of infinity
    _solves(A, dev, [5, 5])
    assert A.rebuilds == []
    dev.kappa[0] = 6.0e-13
    _solves(A, dev, [5])
    assert A.rebuilds == [5]
    for bad in (np.nan, np.inf):
        A, dev = _setup(k0), KappaDev([0.0, 1.0, bad])
        _solves(A, dev, [5])
        assert A.rebuilds == [1] and A.refreshes == 1


def test_iteration_counts_rebuild_the_hierarchy(monkeypatch):
    monkeypatch.delenv("KNP_AMG_REFRESH_EVERY", raising=False)
    k0 = np.ones(3)
    A, dev = _setup(k0), KappaDev(k0)
    h = _solves(A, dev, [9, 5, 4])
    assert A.refresh == {"solves": 3, "ref": 4, "high": 0}                # the smaller of the last two counts, once three solves are in
    _solves(A, dev, [15] * 9, h)                                          # 15 > 3 * 4 + 2
    assert A.refresh["high"] == 9 and A.rebuilds == []
    _solves(A, dev, [14], h)                                              # not above: the run of high counts starts over
    assert A.refresh["high"] == 0
    _solves(A, dev, [15] * 9, h)
    assert A.rebuilds == []
    _solves(A, dev, [15], h)
    assert A.rebuilds == [23] and A.refreshes == 1 and A.refresh == {"solves": 0, "ref": None, "high": 0}
    A = _setup(k0)
    _solves(A, dev, [0, 0, 0])
    assert A.refresh["ref"] == 1                                          # never below one iteration


def test_a_partitioned_run_keeps_its_hierarchy(monkeypatch):
    monkeypatch.setenv("KNP_AMG_REFRESH_EVERY", "1")
    A, dev = _setup(np.ones(3), local_mesh=object()), KappaDev([5.0, np.nan, 1.0])
    _solves(A, dev, [4, 4, 4] + [100] * 12)
    assert A.rebuilds == [] and A.refreshes == 0 and A.refresh == {"solves": 0, "ref": None, "high": 0}


def test_refresh_state_round_trip(monkeypatch):
    monkeypatch.setenv("KNP_AMG_REFRESH_EVERY", "6")
    k0 = np.ones(3)
    A, dev = _setup(k0), KappaDev(2.0 * k0)
    fresh = AmgSetup(A.inp)
    assert fresh.state() == {"solves": 0, "ref": None, "high": 0, "refreshes": 0}
    _solves(A, dev, [4, 4, 4, 20, 20, 20, 4, 4, 4, 20])
    st = A.state()
    assert st == {"solves": 4, "ref": 4, "high": 1, "refreshes": 1}
    assert list(st) == ["solves", "ref", "high", "refreshes"] and all(type(st[k]) is int for k in st)      # the header entry as it is written
    fresh.restore(st)
    assert fresh.state() == st and fresh.refresh == A.refresh and fresh.refreshes == 1
    fresh.restore(None)                                                   # a file from before the entry: counters start over
    assert fresh.state() == {"solves": 0, "ref": None, "high": 0, "refreshes": 1}
    fresh.restore({"solves": 2})
    assert fresh.state() == {"solves": 2, "ref": None, "high": 0, "refreshes": 1}


# ---- effective solver settings --------------------------------------------------------------------------------------------------------
def _sp(**fields):
    return namedtuple("solver_params", tuple(fields))(*fields.values())


def _resolve(sp=None, environ=None, degree=1, direct_emi=False, direct_knp=False):
    return resolve_settings(sp if sp is not None else _sp(), degree_emi=degree, rtol_emi=None if direct_emi else 1e-5,
                            atol_emi=None if direct_emi else 1e-40, rtol_knp=None if direct_knp else 1e-7,
                            atol_knp=None if direct_knp else 2e-40, direct_emi=direct_emi, direct_knp=direct_knp, environ=environ or {})


def test_default_settings():
    for degree in (1, 2):
        s = _resolve(degree=degree)
        assert s.emi_target == (EMI_TARGET_SAFETY / degree ** 2) * (0.1 * 1e-5)
        assert s.rtol_emi == PHI_ENERGY_FACTOR * 1e-5 and s.atol_emi == 1e-40
        assert s.rtol_knp == 1e-7 and s.atol_knp == 2e-40
        assert (s.knp_krylov, s.gmres_restart, s.knp_min_it, s.knp_early) == ("bicgstab", 30, 4, 0.01)
        assert (s.max_it_emi, s.max_it_knp) == (50000, 5000)
    assert type(s.knp_min_it) is int and type(s.gmres_restart) is int and type(s.max_it_emi) is int
    assert s._fields == ("max_it_emi", "max_it_knp", "rtol_emi", "atol_emi", "emi_target", "rtol_knp", "atol_knp", "knp_krylov",
                         "gmres_restart", "knp_min_it", "knp_early")
    assert resolve_settings(None, degree_emi=1, rtol_emi=1e-5, atol_emi=1e-40, rtol_knp=1e-7, atol_knp=2e-40, direct_emi=False,
                            direct_knp=False, environ={}) == _resolve()                                   # no solver_params at all
    s = _resolve(_sp(max_it_emi=200, max_it_knp=30.0))
    assert (s.max_it_emi, s.max_it_knp) == (200, 30)


@pytest.mark.parametrize("sp,environ,want", [
    (dict(knp_krylov="gmres"), {}, dict(knp_krylov="gmres", knp_min_it=5, gmres_restart=30)),
    (dict(), {"KNP_KNP_KRYLOV": "gmres", "KNP_GMRES_RESTART": "20"}, dict(knp_krylov="gmres", knp_min_it=5, gmres_restart=20)),
    (dict(knp_krylov="gmres", gmres_restart=40, knp_min_it=3), {"KNP_GMRES_RESTART": "20"},
     dict(knp_krylov="gmres", gmres_restart=40, knp_min_it=3)),
    (dict(emi_rtol_scale=2e-3), {}, dict(emi_target=None, rtol_emi=max(1e-5 * 2e-3, min(1e-5, 1e-11)))),
    (dict(), {"KNP_EMI_RTOL_SCALE": "2e-3"}, dict(emi_target=None, rtol_emi=max(1e-5 * 2e-3, 1e-11))),
    (dict(emi_rtol_scale=1e-8), {}, dict(emi_target=None, rtol_emi=1e-11)),                              # the floor min(rt, 1e-11)
    (dict(knp_rtol_scale=0.03), {}, dict(rtol_knp=1e-7 * 0.03)),
    (dict(), {"KNP_KNP_RTOL_SCALE": "0.03"}, dict(rtol_knp=1e-7 * 0.03)),
    (dict(knp_rtol_scale=1e-9), {}, dict(rtol_knp=1e-13)),                                               # the floor min(rk, 1e-13)
    (dict(c_tol=3e-7, emi_target_safety=5.0, emi_energy_factor=0.25), {}, dict(emi_target=5.0 * 3e-7, rtol_emi=0.25 * 1e-5)),
    (dict(), {"KNP_EMI_TARGET_SAFETY": "5", "KNP_EMI_ENERGY_FACTOR": "0.25"}, dict(emi_target=5.0 * (0.1 * 1e-5), rtol_emi=0.25 * 1e-5)),
    (dict(), {"KNP_KNP_MIN_IT": "9", "KNP_KNP_EARLY": "0.1"}, dict(knp_min_it=9, knp_early=0.1)),
    # a field beats the variable
    (dict(knp_min_it=7, knp_early_stop=0.5), {"KNP_KNP_MIN_IT": "9", "KNP_KNP_EARLY": "0.1"}, dict(knp_min_it=7, knp_early=0.5)),
    (dict(emi_rtol_scale=2e-3, knp_rtol_scale=0.5), {"KNP_EMI_RTOL_SCALE": "1", "KNP_KNP_RTOL_SCALE": "1"},
     dict(emi_target=None, rtol_emi=1e-5 * 2e-3, rtol_knp=1e-7 * 0.5)),
    (dict(emi_target_safety=5.0, knp_krylov="bicgstab"), {"KNP_EMI_TARGET_SAFETY": "7", "KNP_KNP_KRYLOV": "gmres"},
     dict(emi_target=5.0 * (0.1 * 1e-5), knp_krylov="bicgstab", knp_min_it=4)),
    # a falsy field counts as unset where today's code tests it with `or` ...
    (dict(knp_min_it=0), {}, dict(knp_min_it=4)),
    (dict(knp_min_it=0, gmres_restart=0, c_tol=0.0, emi_target_safety=0, emi_energy_factor=0.0, knp_krylov=""),
     {"KNP_KNP_MIN_IT": "6", "KNP_GMRES_RESTART": "10"},
     dict(knp_min_it=6, gmres_restart=10, emi_target=EMI_TARGET_SAFETY * (0.1 * 1e-5), rtol_emi=PHI_ENERGY_FACTOR * 1e-5,
          knp_krylov="bicgstab")),
    # ... and is a value where it tests `is None`: knp_early_stop = 0 switches the early stop off
    (dict(knp_early_stop=0), {"KNP_KNP_EARLY": "0.1"}, dict(knp_early=0.0)),
    (dict(knp_early_stop=None, emi_rtol_scale=None, knp_rtol_scale=None), {"KNP_KNP_EARLY": "0.1"},
     dict(knp_early=0.1, rtol_emi=PHI_ENERGY_FACTOR * 1e-5, rtol_knp=1e-7)),
])
def test_settings_from_fields_and_variables(sp, environ, want):
    s = _resolve(_sp(**sp), environ)
    base = _resolve()._asdict()
    base.update(want)
    assert s._asdict() == base


def test_direct_solves_are_tight_iterative_ones():
    s = _resolve(direct_emi=True)
    assert s.rtol_emi == 1e-10 and s.atol_emi == 1e-40 and s.emi_target is None and s.rtol_knp == 1e-7 and s.knp_early == 0.01
    s = _resolve(_sp(rtol_direct=1e-12, emi_rtol_scale=2e-3), direct_emi=True)
    assert s.rtol_emi == 1e-12 and s.emi_target is None
    s = _resolve(direct_knp=True)
    assert s.rtol_knp == 1e-10 / 20.0 and s.atol_knp == 1e-40 and s.knp_early == 0.0 and s.emi_target is not None
    s = _resolve(_sp(rtol_direct=1e-12, knp_early_stop=0.5, knp_rtol_scale=0.03), {"KNP_KNP_EARLY": "0.1"}, direct_knp=True)
    assert s.rtol_knp == 1e-12 / 20.0 and s.knp_early == 0.0
