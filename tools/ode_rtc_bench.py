#!/usr/bin/env python3
"""Cost of a runtime-compiled membrane model (HIP_RHS, knpemidg/ode_rtc.py) against the built-in device kernel and the host path.

On all membrane facets of the 3D idealized 4-axon mesh (default r=2, the bench.py mesh: 23 552 facets):
  - one ODE step (dt = 1e-4, stimulus on x < 20 um) of the built-in mm_hh (device id 1), of the same HH written as HIP_RHS
    (examples/custom_membrane_model/mm_hh_rtc.py) and of the host integrate_batch on mm_hh.rhs; device times from stream events
    over --ode-steps steps after warm-up, host times from the wall clock;
  - the hipRTC compile time (uncached) and the compiler's VGPR / scratch figures of both HIP_RHS models;
  - --solver-steps full solver steps (after one warm-up step) of the default run (built-in HH on tags 1 and 2) and of the
    example model (mm_hh_q10 on tag 1, built-in mm_hh_no_stim on tag 2) on the device and under KNP_HOST_ODE=1.
Prints one JSON line; OUT_DIR (default bench_out) receives ode_rtc_bench.json.

    python tools/ode_rtc_bench.py [--resolution 2] [--ode-steps 20] [--solver-steps 20] [--no-solver]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "examples", "idealized_geometries"),
          os.path.join(ROOT, "examples", "custom_membrane_model")):
    if p not in sys.path:
        sys.path.insert(0, p)


def ode_steps(resolution, n_dev, n_host):
    from knpemidg import _abi, ode_rtc
    from knpemidg.functions import FacetSpace, FacetFunction
    from knpemidg.membrane import MembraneModel
    from knpemidg.mesh import make_mesh_3D
    from knpemidg.models import mm_hh
    import mm_hh_q10
    import mm_hh_rtc
    out = {}
    # uncached: past the process memo, and with an empty compiler cache (comgr keeps one on disk unless told otherwise)
    cache = tempfile.mkdtemp()
    old = os.environ.get("AMD_COMGR_CACHE_DIR")
    os.environ["AMD_COMGR_CACHE_DIR"] = cache
    try:
        for name, ode in (("hh_rtc", mm_hh_rtc), ("hh_q10", mm_hh_q10)):
            src, kernel, _, _ = ode_rtc.source(ode)
            t0 = time.perf_counter()
            code, log = ode_rtc._hiprtc(src, kernel)
            out["compile_s_" + name] = time.perf_counter() - t0
            out["resources_" + name] = dict(ode_rtc.resource_usage(log), kernel=kernel, code_bytes=len(code))
    finally:
        if old is None:
            os.environ.pop("AMD_COMGR_CACHE_DIR", None)
        else:
            os.environ["AMD_COMGR_CACHE_DIR"] = old
        shutil.rmtree(cache, ignore_errors=True)
    m, s, f = make_mesh_3D(resolution, n_axons=4)
    dev = _abi.Device(m, s.array(), f.array(), [1, 2], 3)
    f.array()[f.array() == 2] = 1                                  # one model on the membrane facets of all four axons
    Q = FacetSpace(m)
    fields = {'K_e': 3.32, 'Na_i': 12.8, 'E_K': -0.0936, 'E_Na': 0.0533}
    stim = {'stim_amplitude': 10.0}
    locator = lambda x: x[0] < 20.0e-6

    def model(ode, on_dev):
        mm = MembraneModel(ode, facet_f=f, tag=1, V=Q)
        mm.set_parameter_values({'Cm': lambda x: 0.02})
        if on_dev:
            assert mm.attach_device(dev)
        for k, v in fields.items():
            mm.set_parameter(k, FacetFunction(Q, np.full(Q.dim(), v)))
        return mm
    out["membrane_facets"] = model(mm_hh, False).nodes
    for name, ode in (("builtin_hh", mm_hh), ("hip_rhs_hh", mm_hh_rtc)):
        mm = model(ode, True)
        for _ in range(3):
            mm.step_lsoda(dt=1e-4, stimulus=stim, stimulus_locator=locator)
        dev.sync()
        dev.timer_begin()
        for _ in range(n_dev):
            mm.step_lsoda(dt=1e-4, stimulus=stim, stimulus_locator=locator)
        out["ode_step_ms_" + name] = dev.timer_end() / n_dev
        out["v_max_" + name] = float(mm.states[:, 3].max())
    mm = model(mm_hh, False)
    mm.step_lsoda(dt=1e-4, stimulus=stim, stimulus_locator=locator)
    t0 = time.perf_counter()
    for _ in range(n_host):
        mm.step_lsoda(dt=1e-4, stimulus=stim, stimulus_locator=locator)
    out["ode_step_ms_host_integrate_batch"] = 1e3 * (time.perf_counter() - t0) / n_host
    out["ratio_hip_rhs_to_builtin"] = out["ode_step_ms_hip_rhs_hh"] / out["ode_step_ms_builtin_hh"]
    dev.close()
    return out


def solver_steps(resolution, steps, models, host_ode):
    from idealized_common import make_solver, solver_parameters, Constant
    os.environ["KNP_HOST_ODE"] = "1" if host_ode else "0"
    t0 = time.perf_counter()
    S = make_solver(dim=3, resolution=resolution, n_axons=4, ode_models=models)
    on_dev = [bool(mm['ode'].on_device) for mm in S.mem_models]
    S._unpack_solver_params(solver_parameters(3, resolution))
    S.save_fields = S.save_solver_stats = False
    S.splitting_scheme = True
    S.setup_varform_emi(); S.setup_varform_knp(); S.setup_solver_emi(); S.setup_solver_knp()
    t_setup = time.perf_counter() - t0
    t = Constant(0.0)
    S.step_membrane_models(0); S.solve_for_time_step(0, t)
    S.dev.sync()
    ode0 = S.ode_solve_timer
    t0 = time.perf_counter()
    for k in range(1, steps + 1):
        S.step_membrane_models(k); S.solve_for_time_step(k, t)
    S.dev.sync()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    res = dict(ms_per_step=ms, ode_ms_per_step=1e3 * (S.ode_solve_timer - ode0) / steps, setup_s=t_setup, on_device=on_dev,
               emi_iters_per_step=float(np.mean(S.emi_niter[-steps:])),
               knp_iters_per_step=float(np.mean([max(n) for n in S.knp_niter[-steps:]])))
    S.dev.close()
    os.environ.pop("KNP_HOST_ODE", None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=2)
    ap.add_argument("--ode-steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--solver-steps", type=int, default=20)
    ap.add_argument("--no-solver", action="store_true")
    args = ap.parse_args()
    out = dict(resolution=args.resolution, ode=ode_steps(args.resolution, args.ode_steps, args.host_steps))
    if not args.no_solver:
        from knpemidg.models import mm_hh, mm_hh_no_stim
        import mm_hh_q10
        out["solver"] = {
            "builtin_hh": solver_steps(args.resolution, args.solver_steps, {1: mm_hh, 2: mm_hh_no_stim}, False),
            "example_hip_rhs": solver_steps(args.resolution, args.solver_steps, {1: mm_hh_q10, 2: mm_hh_no_stim}, False),
            "example_host_ode": solver_steps(args.resolution, args.solver_steps, {1: mm_hh_q10, 2: mm_hh_no_stim}, True),
        }
        sv = out["solver"]
        out["solver"]["ratio_example_to_builtin"] = sv["example_hip_rhs"]["ms_per_step"] / sv["builtin_hh"]["ms_per_step"]
        out["solver"]["ratio_host_ode_to_example"] = sv["example_host_ode"]["ms_per_step"] / sv["example_hip_rhs"]["ms_per_step"]
    line = json.dumps(out)
    print(line)
    d = os.environ.get("OUT_DIR", os.path.join(ROOT, "bench_out"))
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "ode_rtc_bench.json"), "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
