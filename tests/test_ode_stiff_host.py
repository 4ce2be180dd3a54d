"""The stiff membrane-ODE integrator on the host: knpemidg.membrane.integrate_batch_stiff, the numpy restatement of
csrc/ode_stiff.hpp (extrapolated linearly implicit Euler, 8 columns) -- its order, its accuracy on the fast-gate membrane against
scipy's Radau, its stability on Prothero-Robinson, what it saves over the Dormand-Prince integrator, row independence, and the
protocol of the run-time compiled kernels (ode_rtc.source(ode, method))."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rtc_models                                     # noqa: E402
import stiff_models as sm                             # noqa: E402
from knpemidg.membrane import ODE_STIFF_K, integrate_batch, integrate_batch_stiff   # noqa: E402


def _windows(ode, s0, p0, windows, integrate, stim_rows=None, first_on=10, **kw):
    """`windows` windows of sm.WINDOW with the stimulus of sm.stim_schedule imposed at the start of each, as MembraneModel.step_lsoda
    does; the step size is carried from window to window."""
    y, p, h = s0.copy(), p0.copy(), None
    rows = np.ones(len(y), dtype=bool) if stim_rows is None else stim_rows
    col = ode.parameter_indices("stim_amplitude")
    for k in range(windows):
        p[rows, col] = sm.stim_schedule(k, first_on)
        y, h = integrate(ode.rhs, k * sm.WINDOW, (k + 1) * sm.WINDOW, y, p, rtol=1e-8, atol=0.0, h0=h, **kw)
    return y, p, h


def _order(rhs, exact, T, steps):
    errs = [np.abs(integrate_batch_stiff(rhs, 0.0, T, np.array([[1.0, 0.0]]), np.zeros((1, 1)), fixed_h=H)[0] - exact(T)).max()
            for H in steps]
    return errs, [float(np.log2(errs[i] / errs[i + 1])) for i in range(len(errs) - 1)]


def test_order_is_the_number_of_columns():
    """Fixed steps on the plane rotation (solution (cos t, sin t)) over [0, 4], the step halved twice from 1: the observed order of
    each halving is within 0.5 of the nominal order K = 8 (measured 7.59 and 7.82, rising towards 8; errors 6.8e-6 .. 1.6e-10, above
    the table's round-off floor of about 1e-12).  A wrong extrapolation weight leaves order 1.  The nonlinear, non-autonomous
    system around the same solution is further from its asymptotic regime at these errors; over two halvings from 0.8 it shows
    7.7."""
    exact = lambda T: np.array([[np.cos(T), np.sin(T)]])
    errs, orders = _order(sm.rotation_rhs, exact, 4.0, (1.0, 0.5, 0.25))
    print("rotation: errors %s, observed orders %s" % (errs, orders))
    assert ODE_STIFF_K == 8
    assert all(abs(o - ODE_STIFF_K) <= 0.5 for o in orders), orders
    errs, orders = _order(sm.smooth_rhs, exact, 3.2, (0.8, 0.2))
    print("nonlinear: errors %s, observed order %.2f" % (errs, orders[0] / 2))
    assert abs(orders[0] / 2 - ODE_STIFF_K) <= 0.5, orders


@pytest.mark.parametrize("tau", [1e-7, 1e-9])
def test_fast_gate_matches_radau(tau):
    """The fast-gate membrane at tau_q = 1e-4 ms and 1e-6 ms, 50 windows of 0.1 ms through an action potential with the stimulus
    switched on at the start of window 10, against scipy's Radau at rtol 1e-12 / atol 1e-14: every state within 1e-6 of its maximum
    along the trajectory (the bound of the device-versus-host ODE checks).  Measured 2.4e-11 and 2.9e-11."""
    s0, p0 = sm.hh_rows(sm.fastgate, 1, tau_q=tau)
    ref, ymax = sm.radau_windows(sm.fastgate, s0, p0, 50)
    st = {}
    y, p, h = _windows(sm.fastgate, s0, p0, 50, integrate_batch_stiff, stats=st)
    err = (np.abs(y - ref) / ymax).max(axis=0)
    print("tau_q %.0e s: scaled error per state %s, %s" % (tau, err, st))
    assert ymax[0, 3] > 0.0                                                # it fired
    assert err.max() <= 1e-6, err
    assert (h > 0).all() and st["accepted"] >= 50 and st["rhs_calls"] >= st["jacobians"] * (s0.shape[1] + 1)


def test_prothero_robinson_is_not_step_limited_by_stability():
    """y' = lambda (y - cos t) - sin t with lambda = -1e6 over [0, 10]: at most 3e4 accepted steps, 1 % of the 3e6 the stability interval
    of Dormand-Prince (about 3.3 / |lambda|) forces.  Measured: 3."""
    st = {}
    y, _ = integrate_batch_stiff(sm.prothero_robinson_rhs, 0.0, 10.0, np.array([[1.0]]), np.array([[-1.0e6]]), rtol=1e-8, atol=0.0,
                                 stats=st)
    print("Prothero-Robinson: %s, error %.3g" % (st, float(y[0, 0] - np.cos(10.0))))
    assert st["accepted"] <= 30000, st
    assert abs(y[0, 0] - np.cos(10.0)) <= 1e-6


def test_robertson_reaches_40():
    """Robertson's problem over [0, 40] from (1, 0, 0) with atol 0: the first trial steps overflow and are rejected, the run ends on
    Radau's solution with mass conserved."""
    from scipy.integrate import solve_ivp
    ode = sm.robertson()
    y0, p = ode.init_state_values()[None, :], ode.init_parameter_values()[None, :]
    st = {}
    with np.errstate(all="ignore"):
        y, _ = integrate_batch_stiff(ode.rhs, 0.0, 40.0, y0, p, rtol=1e-8, atol=0.0, stats=st)
    ref = solve_ivp(lambda t, yy: ode.rhs(np.array([t]), yy[None, :], p)[0], (0.0, 40.0), y0[0], method="Radau", rtol=1e-12, atol=1e-16).y[:, -1]
    print("Robertson: %s, y(40) = %s" % (st, y[0]))
    assert np.abs(y[0] - ref).max() <= 1e-6 * np.abs(ref).max() and abs(y[0, 1] - ref[1]) <= 1e-6 * ref[1]
    assert abs(y.sum() - 1.0) < 1e-12 and st["accepted"] < 1000


def test_fewer_rhs_calls_than_dormand_prince():
    """What the integrator is for: on the tau_q = 1e-4 ms membrane (50 windows, one row) it calls the right-hand side fewer times than
    integrate_batch, both counted through a wrapping rhs.  Measured 6 518 against 121 744: a factor of 18.7."""
    s0, p0 = sm.hh_rows(sm.fastgate, 1, tau_q=1e-7)
    calls = {}

    class Counting:
        rhs = None
        parameter_indices = staticmethod(sm.fastgate.parameter_indices)

    def counted(name):
        calls[name] = 0

        def rhs(t, y, p):
            calls[name] += 1
            return sm.fastgate.rhs(t, y, p)
        ode = Counting()
        ode.rhs = rhs
        return ode
    st = {}
    ys, _, _ = _windows(counted("stiff"), s0, p0, 50, integrate_batch_stiff, stats=st)
    yd, _, _ = _windows(counted("dp5"), s0, p0, 50, integrate_batch)
    print("rhs calls: stiff %d, dp5 %d, ratio %.1f" % (calls["stiff"], calls["dp5"], calls["dp5"] / calls["stiff"]))
    assert calls["stiff"] < calls["dp5"], calls
    assert calls["stiff"] == st["rhs_calls"]                               # the counters count what is called
    assert np.abs(ys - yd).max() <= 1e-6 * np.abs(yd).max()


def test_a_row_does_not_depend_on_the_batch():
    """Row 2 of a batch of 5 distinct rows, integrated alone and inside the batch over 12 windows with the stimulus on part of the
    rows: the same bits in states, currents and step size."""
    s0, p0 = sm.hh_rows(sm.fastgate, 5, tau_q=1e-9)
    rows = np.array([True, False, True, True, False])
    yb, pb, hb = _windows(sm.fastgate, s0, p0, 12, integrate_batch_stiff, stim_rows=rows, first_on=3)
    y1, p1, h1 = _windows(sm.fastgate, s0[2:3], p0[2:3], 12, integrate_batch_stiff, stim_rows=rows[2:3], first_on=3)
    assert y1.tobytes() == yb[2:3].tobytes() and p1.tobytes() == pb[2:3].tobytes() and h1.tobytes() == hb[2:3].tobytes()
    assert np.abs(yb[0] - yb[1]).max() > 1e-3                              # the rows differ


def test_rtc_protocol_of_the_stiff_kernel():
    """source(ode, "stiff") is a translation unit of its own around csrc/ode_stiff.hpp, its kernel name carries the method, the DP5
    unit is what it was; more states than ODE_STIFF_MAX_STATES and an unknown method raise ValueError."""
    from knpemidg import ode_rtc
    from knpemidg.membrane import check_ode_method
    src_d, k_d, ns, npar = ode_rtc.source(sm.fastgate)
    src_s, k_s, ns_s, npar_s = ode_rtc.source(sm.fastgate, "stiff")
    assert (ns, npar) == (ns_s, npar_s) == (5, 19)
    assert k_s.startswith("k_ode_rtc_stiff_mm_hh_fastgate_") and k_d.startswith("k_ode_rtc_mm_hh_fastgate_") and k_s[-8:] != k_d[-8:]
    assert "ode_stiff_step<5, 19>" in src_s and "ode_dp5_step<" not in src_s and "ode_stiff" not in src_d
    assert ode_rtc.source(sm.fastgate, "dp5") == (src_d, k_d, ns, npar)
    assert ode_rtc.STIFF_MAX_STATES == 11
    names = tuple("s%d" % i for i in range(12))
    big = rtc_models.make_model("mm_twelve", "dy[0] = 0.0;", states=names, params=("a",))
    ode_rtc.source(big)                                                    # DP5 takes it
    with pytest.raises(ValueError, match="11"):
        ode_rtc.source(big, "stiff")
    for bad in ("lsoda", "", 1, "Stiff"):
        with pytest.raises(ValueError, match="'dp5', 'stiff'"):
            ode_rtc.source(sm.fastgate, bad)
        with pytest.raises(ValueError, match="'dp5', 'stiff'"):
            check_ode_method(bad)
    assert check_ode_method(None) == "dp5" and sm.fastgate.ODE_METHOD == "stiff"


def test_method_selection_of_model_and_solver():
    """MembraneModel takes the module's ODE_METHOD unless told otherwise and reads it back; Solver.setup_membrane_model refuses an
    unknown method, and a tag without a model, before it touches anything."""
    from knpemidg.functions import FacetSpace
    from knpemidg.membrane import MembraneModel
    from knpemidg.mesh import make_mesh_2D
    from knpemidg.models import mm_hh
    from knpemidg.solver import Solver
    m, s, f = make_mesh_2D(1)
    Q = FacetSpace(m)
    assert MembraneModel(sm.fastgate, facet_f=f, tag=1, V=Q).ode_method == "stiff"
    assert MembraneModel(sm.fastgate, facet_f=f, tag=1, V=Q, ode_method="dp5").ode_method == "dp5"
    assert MembraneModel(mm_hh, facet_f=f, tag=1, V=Q).ode_method == "dp5"
    mm = MembraneModel(mm_hh, facet_f=f, tag=1, V=Q, ode_method="stiff")
    assert mm.ode_method == "stiff" and not mm.on_device and set(mm.ode_stats().values()) == {0}
    mm.set_parameter_values({name: (lambda x, v=v: v) for name, v in sm.HH_ENV.items()})
    v0 = mm.states[:, 3].copy()
    mm.step_lsoda(dt=sm.WINDOW, stimulus={"stim_amplitude": sm.STIM})
    st = mm.ode_stats()
    assert st["accepted"] >= mm.nodes > 0 and st["jacobians"] == st["accepted"] + st["rejected"] and np.abs(mm.states[:, 3] - v0).max() > 1e-4
    with pytest.raises(ValueError, match="'dp5', 'stiff'"):
        MembraneModel(mm_hh, facet_f=f, tag=1, V=Q, ode_method="bdf")
    for bad in ("lsoda", {1: "rk4"}, 3):
        with pytest.raises(ValueError, match="'dp5', 'stiff'"):
            Solver.setup_membrane_model(None, None, {1: mm_hh}, ode_method=bad)
    with pytest.raises(ValueError, match="no membrane model"):
        Solver.setup_membrane_model(None, None, {1: mm_hh}, ode_method={7: "stiff"})
