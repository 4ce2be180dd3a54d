"""The stiff membrane-ODE integrator on the device (csrc/ode_stiff.hpp: k_ode_step_stiff for the built-in models, the run-time
compiled stiff kernel for HIP_RHS models, knp_ode_set_method / knp_ode_register_method / knp_ode_stats): against its host replica
(membrane.integrate_batch_stiff) and scipy's Radau at the kernel level, against the Dormand-Prince kernel on a non-stiff model,
through the Solver against the host-ODE run, and across a checkpoint.

None of this runs on a commit without the method: it cannot be selected there.  The case to point at is the fast-gate model at
tau_q = 1e-6 ms: the Dormand-Prince replica needs 9.4e6 right-hand-side calls for 5 ms of it, about 188 000 per 0.1 ms window, beyond the
kernel's 100 000 steps per launch, so under method 0 the same launch would end in the failure flag (a count made on the host; that
launch is not made here)."""
import os
import sys

import numpy as np
import pytest

import knpemi_oracle as ko
from common import device_for, relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "examples", "idealized_geometries"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import stiff_models as sm                             # noqa: E402

pytestmark = pytest.mark.gpu

WINDOWS, FIRST_ON = 20, 5


@pytest.fixture(scope="module")
def dev(hip_lib):
    from knpemidg.mesh import make_mesh_2D
    m, s, f = make_mesh_2D(1)
    d = device_for(ko.build_idealized(m, s.array(), f.array(), membrane_tags=(1,)))
    yield d
    d.close()


def _hstore(dev, handle):
    """step size of every node of a set, from the device snapshot (state block 1000 + 8 handle + 2, csrc/ode.hip)"""
    from knpemidg import checkpoint
    table, arrays = checkpoint.split_snapshot(dev.state_save())
    return arrays[[int(b["id"]) for b in table].index(1000 + 8 * handle + 2)].ravel()


def _device_windows(dev, model, ode, s8, p8, n, method, windows=WINDOWS):
    """n nodes = the 8 rows tiled, the stimulus (off, then on from window FIRST_ON) on every third node; returns states, parameters,
    counters and the step sizes after the first and the last window."""
    rows = np.arange(n) % 8
    mask = np.arange(n) % 3 == 0
    ns, npar = s8.shape[1], p8.shape[1]
    h = dev.ode_create(model, (np.arange(n) % dev.nf).astype(np.int32), s8[rows].reshape(n, ns), p8[rows].reshape(n, npar))
    dev.ode_set_method(h, method)
    col = ode.parameter_indices("stim_amplitude")
    h_first = None
    for k in range(windows):
        dev.ode_set_stimulus(h, [col], [sm.stim_schedule(k, FIRST_ON)], mask)
        dev.ode_step(h, k * sm.WINDOW, sm.WINDOW, rtol=1e-8, atol=0.0)
        if k == 0 and n:
            h_first = _hstore(dev, h)
    out = dict(states=dev.ode_table(h, 0, (n, ns)), params=dev.ode_table(h, 1, (n, npar)), stats=dev.ode_stats(h), h_first=h_first,
               h_last=_hstore(dev, h) if n else None, mask=mask, handle=h)
    dev.sync()
    return out


def _host_windows(ode, s, p, mask, windows=WINDOWS):
    from knpemidg.membrane import integrate_batch_stiff
    y, p, h = s.copy(), p.copy(), None
    col = ode.parameter_indices("stim_amplitude")
    for k in range(windows):
        p[mask, col] = sm.stim_schedule(k, FIRST_ON)
        y, h = integrate_batch_stiff(ode.rhs, k * sm.WINDOW, (k + 1) * sm.WINDOW, y, p, rtol=1e-8, atol=0.0, h0=h)
    return y, p


def _model(dev, which):
    """(device model id, model module, its 8 distinct rows, columns of the channel currents)"""
    if which == "hh":
        from knpemidg.models import mm_hh
        assert mm_hh.MODEL_ID == 1
        return 1, mm_hh, sm.hh_rows(mm_hh, 8), [8, 9]
    ode = sm.fastgate
    return dev.ode_register(ode, "stiff"), ode, sm.hh_rows(ode, 8, tau_q=1.0e-9), [8, 9]


@pytest.mark.parametrize("which", ["hh", "fastgate"])
@pytest.mark.parametrize("n", [0, 1, 130])
def test_stiff_kernel_matches_replica_and_radau(dev, which, n):
    """Built-in HH under method 1 and the run-time compiled fast-gate model at tau_q = 1e-6 ms, 0 / 1 / 130 nodes (two full blocks of 64
    and a tail) made of 8 distinct rows, 20 windows of 0.1 ms with the stimulus switched on at window 5 on every third node.
    States within 1e-6 and currents within 1e-5 of their maximum of the host replica (the bounds of the device-versus-host checks of
    tests/test_gpu_ode_rtc.py); the first 8 nodes within 1e-6 per state, scaled by the trajectory's maximum, of Radau at rtol 1e-12;
    nodes that tile the same row and stimulus bitwise equal; the step size positive and carried; the counters consistent."""
    model, ode, (s8, p8), cur = _model(dev, which)
    ns = s8.shape[1]
    out = _device_windows(dev, model, ode, s8, p8, n, 1)
    sd, pd, stats = out["states"], out["params"], out["stats"]
    if n == 0:
        assert sd.shape == (0, ns) and (stats == 0).all()
        return
    m = min(n, 24)                                     # (row, stimulus) repeats with period lcm(8, 3)
    rows = np.arange(m) % 8
    sh, ph = _host_windows(ode, s8[rows], p8[rows], out["mask"][:m])
    e_s = np.abs(sd[:m] - sh).max() / np.abs(sh).max()
    e_c = np.abs(pd[:m, cur] - ph[:, cur]).max() / np.abs(ph[:, cur]).max()
    k = min(n, 8)
    ref, ymax = sm.radau_windows(ode, s8, p8, WINDOWS, stim_rows=np.arange(8) % 3 == 0, first_on=FIRST_ON)
    e_r = (np.abs(sd[:k] - ref[:k]) / ymax[:k]).max(axis=0)
    print("%s n=%d: vs replica states %.3g currents %.3g, vs Radau per state %s, counters %s" % (which, n, e_s, e_c, e_r, stats))
    assert e_s <= 1e-6, e_s
    assert e_c <= 1e-5, e_c
    assert e_r.max() <= 1e-6, e_r
    for i in range(24, n):
        assert sd[i].tobytes() == sd[i - 24].tobytes() and pd[i].tobytes() == pd[i - 24].tobytes(), i
    h1, h2 = out["h_first"], out["h_last"]
    assert h1.shape == (n,) and (h1 > 0).all() and (h2 > 0).all()
    assert (h2[24:] == h2[:-24]).all()
    assert not (h2 == sm.WINDOW / 16).all()            # not the start value of a set without history
    acc, rej, nrhs, njac = (int(v) for v in stats)
    assert acc >= n * WINDOWS and rej >= 0 and njac == acc + rej
    assert nrhs >= njac * (ns + 1) and nrhs == njac * (1 + ns + 36) + n * WINDOWS
    if n > 1:
        assert ymax[0, ode.state_indices("V")] > 0.0 and np.abs(sd[0] - sd[1]).max() > 1e-3     # a stimulated row fired, an unstimulated one did not


def test_hh_agrees_under_both_methods(dev):
    """Built-in HH, the same 130 nodes and windows under method 0 (Dormand-Prince) and method 1: within 1e-6 of the maximum.  Only the
    stiff kernel counts; an unknown method is refused and leaves the set as it was."""
    from knpemidg import _abi
    model, ode, (s8, p8), cur = _model(dev, "hh")
    a = _device_windows(dev, model, ode, s8, p8, 130, 0)
    b = _device_windows(dev, model, ode, s8, p8, 130, 1)
    err = np.abs(a["states"] - b["states"]).max() / np.abs(a["states"]).max()
    print("HH dp5 vs stiff: %.3g; stiff counters %s" % (err, b["stats"]))
    assert err <= 1e-6, err
    assert np.abs(a["params"][:, cur] - b["params"][:, cur]).max() <= 1e-5 * np.abs(a["params"][:, cur]).max()
    counted = [0, 2, 3]                                 # accepted, right-hand-side calls, Jacobians (a launch may reject nothing)
    assert (a["stats"] == 0).all() and (b["stats"][counted] > 0).all()
    for bad in (2, -1):
        with pytest.raises(_abi.KnpError, match="knp_ode_set_method"):
            dev.ode_set_method(b["handle"], bad)
    before = dev.ode_stats(b["handle"])
    dev.ode_step(b["handle"], WINDOWS * sm.WINDOW, sm.WINDOW)
    assert (dev.ode_stats(b["handle"])[counted] > before[counted]).all()       # still the stiff kernel


# ---------------------------------------------------------------------------------------------------------------- through the Solver
STEPS = 5


def _make(monkeypatch, host_ode=False, ode_method=None):
    from idealized_common import make_solver, solver_parameters
    from knpemidg.models import mm_hh_no_stim
    monkeypatch.setenv("KNP_NO_AMG", "1")
    monkeypatch.setenv("KNP_HOST_ODE", "1" if host_ode else "0")
    S = make_solver(dim=3, resolution=0, n_axons=4, ode_models={1: sm.fastgate, 2: mm_hh_no_stim}, ode_method=ode_method)
    S._unpack_solver_params(solver_parameters(3, 0, emi_dg_chebyshev=True))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    return S


def _snap(S):
    out = {"c": S.c.array().copy(), "phi": S.phi.array().copy(), "phi_M": S.phi_M_prev_PDE.array().copy(),
           "emi_niter": np.asarray(S.emi_niter), "knp_niter": np.asarray(S.knp_niter).ravel()}
    for i, m in enumerate(S.mem_models):
        out["states_%d" % i] = np.array(m['ode'].states, copy=True)
        out["params_%d" % i] = np.array(m['ode'].parameters, copy=True)
    return out


def _steps(S, k0, k1, t, save_after=None, path=None):
    snaps = []
    for k in range(k0, k1):
        S.step_membrane_models(k)
        S.solve_for_time_step(k, t)
        snaps.append(_snap(S))
        if save_after is not None and k + 1 == save_after:
            S.save_checkpoint(path)
    return snaps


_device_run = {}


def _run_on_device(monkeypatch, tmp_path_factory):
    """The uninterrupted 5-step run with the fast-gate model as a run-time compiled stiff model on tag 1 (shared by the tests below):
    snapshots after every step and a checkpoint written after step 2."""
    if not _device_run:
        from idealized_common import Constant
        S = _make(monkeypatch)
        mm = S.mem_models[0]['ode']
        assert [m['ode'].on_device for m in S.mem_models] == [True, True]
        assert mm.ode_method == "stiff" and S.mem_models[1]['ode'].ode_method == "dp5"
        path = str(tmp_path_factory.mktemp("ode_stiff") / "ck.h5")
        _device_run.update(snaps=_steps(S, 0, STEPS, Constant(0.0), save_after=2, path=path), path=path, stats=mm.ode_stats(),
                           other=S.mem_models[1]['ode'].ode_stats(), nodes=mm.nodes, idx=mm.indices.copy(),
                           header=S._checkpoint_header()["models"])
        S.dev.close()
    return _device_run


def test_solver_with_stiff_model_matches_host_ode_run(hip_lib, monkeypatch, tmp_path_factory):
    """The 3D r=0 4-axon mesh, 5 steps without AMG, the fast-gate model (tau_q = 1e-6 ms) on tag 1 and the built-in mm_hh_no_stim on tag
    2: as a run-time compiled stiff model on the device against the same run under KNP_HOST_ODE=1 (integrate_batch_stiff):
    concentrations within 1e-6 and phi_M within 1e-4 (the bounds of tests/test_gpu_ode_rtc.py)."""
    from idealized_common import Constant
    D = _run_on_device(monkeypatch, tmp_path_factory)
    H = _make(monkeypatch, host_ode=True)
    assert [m['ode'].on_device for m in H.mem_models] == [False, False] and H.mem_models[0]['ode'].ode_method == "stiff"
    h = _steps(H, 0, STEPS, Constant(0.0))[-1]
    host_stats = H.mem_models[0]['ode'].ode_stats()
    H.dev.close()
    d = D["snaps"][-1]
    print("c %.3g, phi_M %.3g; device counters %s, host counters %s" % (relerr(d["c"], h["c"]), relerr(d["phi_M"], h["phi_M"]), D["stats"], host_stats))
    assert relerr(d["c"], h["c"]) < 1e-6, relerr(d["c"], h["c"])
    assert relerr(d["phi_M"], h["phi_M"]) < 1e-4, relerr(d["phi_M"], h["phi_M"])
    assert np.abs(d["phi_M"][D["idx"]] - D["snaps"][0]["phi_M"][D["idx"]]).max() > 1e-4      # the membrane moved
    assert D["stats"]["accepted"] >= STEPS * D["nodes"] and D["stats"]["jacobians"] == D["stats"]["accepted"] + D["stats"]["rejected"]
    assert host_stats["accepted"] >= STEPS * D["nodes"] and set(D["other"].values()) == {0}


def test_checkpoint_resumes_bitwise_and_refuses_the_other_method(hip_lib, monkeypatch, tmp_path_factory):
    """The run above saved after step 2 and resumed in a new Solver: steps 3-5 bit for bit those of the uninterrupted run (the step
    sizes travel in the device snapshot).  The header names the method only where it is not the default, and a Solver that would
    integrate tag 1 with the other method refuses the file, naming `models`; so does one that changes the built-in model's."""
    from idealized_common import Constant
    from knpemidg import _abi
    D = _run_on_device(monkeypatch, tmp_path_factory)
    assert [m.get("ode_method") for m in D["header"]] == ["stiff", None] and "ode_method" not in D["header"][1]
    B = _make(monkeypatch)
    t = Constant(0.0)
    assert B.load_checkpoint(D["path"], t=t) == 2
    resumed = _steps(B, 2, STEPS, t)
    B.dev.close()
    for j, b in enumerate(resumed):
        a = D["snaps"][2 + j]
        for key in a:
            assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), ("step", 3 + j, key, np.abs(a[key] - b[key]).max())
    for other in ({1: "dp5"}, {2: "stiff"}):
        C = _make(monkeypatch, ode_method=other)
        with pytest.raises(_abi.KnpError, match="models"):
            C.load_checkpoint(D["path"])
        C.dev.close()
