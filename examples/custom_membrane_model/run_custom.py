#!/usr/bin/python3
"""3D idealized geometry (r=0, 4 axons) with a user-written membrane model on the stimulated axon: mm_hh_q10 (HH with Q10
temperature scaling and a persistent Na current) on tag 1, the built-in mm_hh_no_stim on tag 2.  mm_hh_q10 has no built-in
device id; its HIP_RHS is compiled at set-up and integrated on the GPU (KNP_HOST_ODE=1 runs it on the host instead).

    python run_custom.py [Tstop] [--stiff]

--stiff puts mm_hh_fastgate on tag 1 instead: HH with a persistent Na current whose gate relaxes in 1e-9 s, a stiff model that
asks for the extrapolated linearly implicit Euler integrator (ODE_METHOD = "stiff") and prints its step counters."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "idealized_geometries"))
sys.path.insert(0, HERE)

from idealized_common import make_solver, solver_parameters, Constant   # noqa: E402
from knpemidg.models import mm_hh_no_stim                                 # noqa: E402
import mm_hh_q10                                                          # noqa: E402

if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--stiff"]
    stiff = "--stiff" in sys.argv[1:]
    Tstop = float(args[0]) if args else 2.0e-3
    if stiff:
        import mm_hh_fastgate
    S = make_solver(dim=3, resolution=0, n_axons=4, ode_models={1: mm_hh_fastgate if stiff else mm_hh_q10, 2: mm_hh_no_stim})
    for mm in S.mem_models:
        print("tag %d: %s on the %s, integrator %s" % (mm['ode'].tag, mm['ode'].prefix, "device" if mm['ode'].on_device else "host",
                                                        mm['ode'].ode_method))
    t = Constant(0.0)
    S.solve_system_active(Tstop, t, solver_parameters(3, 0), filename="results/data/custom/", save_fields=False,
                          save_solver_stats=False)
    phi_M = S.phi_M_prev_PDE.array()
    idx = S.mem_models[0]['ode'].indices
    print("steps %d, ODE time %.3f s; phi_M on tag 1: min %.2f mV, max %.2f mV"
          % (len(S.emi_niter), S.ode_solve_timer, 1e3 * phi_M[idx].min(), 1e3 * phi_M[idx].max()))
    if stiff:
        print("stiff integrator on tag 1: %s" % S.mem_models[0]['ode'].ode_stats())
