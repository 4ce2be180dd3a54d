"""User-written membrane models on the device (HIP_RHS compiled at run time, knpemidg/ode_rtc.py + knp_ode_register): the
same integrator as the built-in models (csrc/ode_dp5.hpp), checked against the built-in HH kernel, against the host integrator
for model sizes no built-in has, and in the full solver against the host-ODE run."""
import os
import sys

import numpy as np
import pytest

import knpemi_oracle as ko
from common import device_for, relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "custom_membrane_model"))
sys.path.insert(0, os.path.join(ROOT, "examples", "idealized_geometries"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rtc_models                                     # noqa: E402

pytestmark = pytest.mark.gpu


def _mesh_2d():
    from knpemidg.mesh import make_mesh_2D
    m, s, f = make_mesh_2D(1)
    return m, s, f, ko.build_idealized(m, s.array(), f.array(), membrane_tags=(1,))


def test_hip_rhs_hh_matches_built_in_hh(hip_lib):
    """mm_hh written as HIP_RHS (examples/custom_membrane_model/mm_hh_rtc.py) against the built-in kernel k_ode_step<1,4,17>:
    rows, fields and stimulus mask of test_device_ode_matches_lsoda_oracle, 25 steps through the upstroke.  The two kernels
    are the same instructions (same integrator text, same right-hand side operation by operation, same code generation
    settings), so the results are expected bitwise; the bound is 1e-10 relative."""
    import mm_hh_rtc
    from knpemidg.functions import FacetSpace, FacetFunction
    from knpemidg.membrane import MembraneModel
    from knpemidg.models import mm_hh
    m, s, f, pb = _mesh_2d()
    dev = device_for(pb)
    Q = FacetSpace(m)
    rng = np.random.default_rng(11)
    fields = {'K_e': 3.32 * (1 + 0.1 * rng.uniform(-1, 1, Q.dim())), 'Na_i': 12.8 * (1 + 0.1 * rng.uniform(-1, 1, Q.dim())),
              'E_K': -0.0936 + 2e-3 * rng.uniform(-1, 1, Q.dim()), 'E_Na': 0.0533 + 2e-3 * rng.uniform(-1, 1, Q.dim())}
    locator = lambda x: x[0] < 20e-6
    mms = []
    for ode in (mm_hh, mm_hh_rtc):
        mm = MembraneModel(ode, facet_f=f, tag=1, V=Q)
        mm.set_parameter_values({'Cm': lambda x: 0.02})
        assert mm.attach_device(dev) and mm.on_device
        for name, val in fields.items():
            mm.set_parameter(name, FacetFunction(Q, val))
        mms.append(mm)
    assert mms[1]._handle != mms[0]._handle and dev._rtc_ids
    mask = np.fromiter(map(locator, mms[0].dof_locations), dtype=bool, count=mms[0].nodes)
    assert 0 < mask.sum() < mms[0].nodes
    v0 = mms[0].states[:, 3].copy()
    for k in range(25):
        for mm in mms:
            mm.step_lsoda(dt=1e-4, stimulus={'stim_amplitude': 40.0}, stimulus_locator=locator)
    (sb, pbi), (sr, pr) = [(mm.states, mm.parameters) for mm in mms]
    assert np.abs(sr - sb).max() <= 1e-10 * np.abs(sb).max(), np.abs(sr - sb).max()
    cur = slice(8, 10)
    assert np.abs(pr[:, cur] - pbi[:, cur]).max() <= 1e-10 * np.abs(pbi[:, cur]).max()
    assert sb[mask, 3].max() > -0.05 and np.abs(sb[:, 3] - v0).max() > 1e-2      # the stimulated rows fired
    print("HIP_RHS HH vs built-in HH: bitwise %s (states max diff %.3g)" % (np.array_equal(sr, sb) and np.array_equal(pr, pbi),
                                                                          np.abs(sr - sb).max()))
    dev.close()


def _host_vs_device(dev, f, Q, ode, set_params, locator, stimulus, dt, steps):
    from knpemidg.membrane import MembraneModel
    out = []
    for on_dev in (False, True):
        mm = MembraneModel(ode, facet_f=f, tag=1, V=Q)
        set_params(mm)
        if on_dev:
            assert mm.attach_device(dev) and mm.on_device
        else:
            assert not mm.on_device
        out.append(mm)
    s0 = out[0].states.copy()
    for k in range(steps):
        for mm in out:
            mm.step_lsoda(dt=dt, stimulus=stimulus, stimulus_locator=locator)
    return s0, out


@pytest.mark.parametrize("which", ["fhn", "hh_q10"])
def test_hip_rhs_models_match_host_integrator(hip_lib, which):
    """A model with sizes no built-in has (FitzHugh-Nagumo type, 2 states / 9 parameters, tests/rtc_models.py) and the example
    model (HH with Q10 scaling and a persistent Na current, 4 / 21) against the host integrate_batch on their numpy `rhs`:
    25 steps with the stimulus on part of the rows; the bounds of the device-vs-LSODA tests (1e-6 states, 1e-5 currents)."""
    from knpemidg.functions import FacetSpace, FacetFunction
    m, s, f, pb = _mesh_2d()
    dev = device_for(pb)
    Q = FacetSpace(m)
    rng = np.random.default_rng(7)
    locator = lambda x: x[0] < 20e-6
    if which == "fhn":
        ode = rtc_models.fhn()
        a = 0.7 * (1 + 0.05 * rng.uniform(-1, 1, Q.dim()))

        def set_params(mm):
            mm.set_parameter('a', FacetFunction(Q, a))
        stimulus, dt, iV, cur = {'stim_amplitude': 1.0}, 0.1, 0, [5, 6]
    else:
        import mm_hh_q10 as ode
        fields = {'K_e': 3.32 * (1 + 0.1 * rng.uniform(-1, 1, Q.dim())), 'Na_i': 12.8 * (1 + 0.1 * rng.uniform(-1, 1, Q.dim())),
                  'E_K': -0.0936 + 2e-3 * rng.uniform(-1, 1, Q.dim()), 'E_Na': 0.0533 + 2e-3 * rng.uniform(-1, 1, Q.dim())}

        def set_params(mm):
            mm.set_parameter_values({'Cm': lambda x: 0.02})
            for name, val in fields.items():
                mm.set_parameter(name, FacetFunction(Q, val))
        stimulus, dt, iV, cur = {'stim_amplitude': 40.0}, 1e-4, 3, [8, 9]
    s0, (host, devm) = _host_vs_device(dev, f, Q, ode, set_params, locator, stimulus, dt, 25)
    mask = np.fromiter(map(locator, host.dof_locations), dtype=bool, count=host.nodes)
    assert 0 < mask.sum() < host.nodes
    sh, sd = host.states, devm.states
    ph, pd = host.parameters, devm.parameters
    assert np.abs(sd - sh).max() < 1e-6 * np.abs(sh).max(), np.abs(sd - sh).max()
    assert np.abs(pd[:, cur] - ph[:, cur]).max() < 1e-5 * np.abs(ph[:, cur]).max()
    dv = np.abs(sd[:, iV] - s0[:, iV])
    assert dv.max() > 1e-2 * np.abs(s0[:, iV]).max()                       # the rows moved
    assert dv[mask].max() > 2 * dv[~mask].max()                            # most where the stimulus acts
    dev.close()


def _solver_run(monkeypatch, host_ode):
    import mm_hh_q10
    from idealized_common import make_solver, solver_parameters, Constant
    from knpemidg.models import mm_hh_no_stim
    monkeypatch.setenv("KNP_HOST_ODE", "1" if host_ode else "0")
    S = make_solver(dim=3, resolution=0, n_axons=4, ode_models={1: mm_hh_q10, 2: mm_hh_no_stim})
    on_dev = [mm['ode'].on_device for mm in S.mem_models]
    S._unpack_solver_params(solver_parameters(3, 0))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    t = Constant(0.0)
    for k in range(20):
        S.step_membrane_models(k)
        S.solve_for_time_step(k, t)
    out = (S.c.array().copy(), S.phi_M_prev_PDE.array().copy(), on_dev, S.mem_models[0]['ode'].indices.copy())
    S.dev.close()
    return out


def test_solver_with_hip_rhs_model_matches_host_ode_run(hip_lib, monkeypatch):
    """The 3D r=0 4-axon mesh with the example model (HIP_RHS) on tag 1 and the built-in mm_hh_no_stim on tag 2, 20 steps,
    against the same run under KNP_HOST_ODE=1 (both models on the host integrator): concentrations within 1e-6 and phi_M
    within 1e-4, the project's bounds for runs that differ only in how their ODEs and solves round."""
    c_d, phiM_d, on_d, idx = _solver_run(monkeypatch, False)
    c_h, phiM_h, on_h, _ = _solver_run(monkeypatch, True)
    assert on_d == [True, True] and on_h == [False, False]
    assert relerr(c_d, c_h) < 1e-6, relerr(c_d, c_h)
    assert relerr(phiM_d, phiM_h) < 1e-4, relerr(phiM_d, phiM_h)
    assert phiM_d[idx].max() > -0.07                                       # the stimulated axon depolarised


def test_two_devices_compile_once_and_both_run(hip_lib, monkeypatch):
    """The code object is memoised per process: two contexts register the same compile (hipRTC runs once) and both step."""
    from knpemidg import ode_rtc
    from knpemidg.functions import FacetSpace
    from knpemidg.membrane import MembraneModel
    calls = []
    real = ode_rtc._hiprtc

    def counting(src, kernel):
        calls.append(kernel)
        return real(src, kernel)
    monkeypatch.setattr(ode_rtc, "_hiprtc", counting)
    ode = rtc_models.make_model("mm_fhn_two_devices", rtc_models.FHN_BODY, s0=[-1.1994, -0.6243],
                                p0=[0.7, 0.8, 12.5, 1.0, 0.5, 0.0, 0.0, 0.0, 1.0], rhs=rtc_models.fhn_rhs)
    m, s, f, pb = _mesh_2d()
    Q = FacetSpace(m)
    results = []
    devs = [device_for(pb), device_for(pb)]
    for dev in devs:
        mm = MembraneModel(ode, facet_f=f, tag=1, V=Q)
        assert mm.attach_device(dev) and mm.on_device
        s0 = mm.states.copy()
        for k in range(5):
            mm.step_lsoda(dt=0.1, stimulus=None)
        results.append(mm.states)
        assert np.abs(results[-1] - s0).max() > 1e-3
    assert len(calls) == 1, calls
    assert np.array_equal(results[0], results[1])
    for dev in devs:
        dev.close()
