#!/usr/bin/python3
"""The run_3D.py configuration with the traces of the reference's figure script recorded on the device instead of per-step field
output (reference: examples/idealized-geometries/make_figures_3D.py:179-194): phi and the concentrations at one intracellular and
one extracellular point, the area-averaged phi_M / E_k / I_ch_k over the membrane facets of a small box, and the subdomain integrals.
Also what the reference's rat-neuron figure script derives from saved fields (examples/rat-neuron/make_figures_rat_neuron.py:238-315,
423-692): the gating variables n, m, h averaged over two boxes of membrane facets, a per-facet activation map of the whole membrane
and the conduction velocity between the two boxes.  Writes results/data/3D/timeseries.h5 and no fields.

    python run_3D_traces.py [resolution] [Tstop]

On several GPUs it is launched the way bench.py is, one process per rank (torchrun --nproc-per-node N run_3D_traces.py ...): with
WORLD_SIZE > 1 the solver is partitioned (knpemidg.partition.make_distributed_solver), every rank makes the same record() call in the
global mesh's terms, the partial rows are summed over the ranks when they are read, and rank 0 prints and writes the file.  With
KNP_COMM_SHM=/name set, the ranks may share one GPU (validation transport, no torch.distributed needed).
"""
import os
import sys

import numpy as np

from idealized_common import make_solver, solver_parameters, Constant

UM = 1.0e-6          # the figure script works in micrometres, the mesh is in metres

if __name__ == "__main__":
    resolution = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    Tstop = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0e-2
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch
        from knpemidg.partition import make_distributed_solver
        local_rank, dist = int(os.environ.get("LOCAL_RANK", "0")), None
        if os.environ.get("KNP_COMM_SHM"):
            local_rank %= torch.cuda.device_count()
        else:
            import torch.distributed as dist
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))     # carries the RCCL ids to the ranks
        S = make_distributed_solver(dim=3, resolution=resolution, rank=rank, world=world, local_rank=local_rank, dist=dist)
    else:
        S = make_solver(dim=3, resolution=resolution, verbose=False)
    x_i, x_e = (25.0, 0.3, 0.3), (25.0, 0.45, 0.65)                    # make_figures_3D.py:181-183
    x_M = np.array([25.6, 0.34, 0.4])                                  # make_figures_3D.py:179, box of :95-97
    eps = 1.0e-6                                                       # the membrane plane z = 0.4 is a rounded grid coordinate
    box = ((x_M - [0.0, 0.01, 0.01]) * UM, (x_M + [0.5, eps, eps]) * UM)
    shift = np.array([4.0, 0.0, 0.0]) * UM                             # a second box 4 um upstream, also outside the stimulated x < 20 um
    box_up = (box[0] - shift, box[1] - shift)
    rec = S.record(points=np.array([x_i, x_e]) * UM, membrane_sets=[box, box_up], regions=True, membrane_states=("n", "m", "h"),
                   membrane_map=dict(threshold=0.0))
    t = Constant(0.0)
    S.solve_system_active(Tstop, t, solver_parameters(3, resolution), filename="results/data/3D/", save_fields=False,
                          save_solver_stats=False)
    # the reads below are collective in a partitioned run: every rank makes them, rank 0 prints
    say = print if rank == 0 else (lambda *a: None)
    phi_M = 1.0e3 * rec.membrane["phi_M"][:, 0]
    k = int(np.argmax(phi_M))
    say("steps %d  membrane set of %d facets  phi_M peak %.3f mV at t = %.2f ms  (E_K %.2f mV, E_Na %.2f mV there)"
        % (len(rec.t), len(rec.set_facets[0]), phi_M[k], 1.0e3 * rec.t[k], 1.0e3 * rec.membrane["E_K"][k, 0],
           1.0e3 * rec.membrane["E_Na"][k, 0]))
    say("intracellular probe: K %.4f -> %.4f mM, extracellular probe: K %.4f -> %.4f mM"
        % (rec.points["K"][0, 0], rec.points["K"][-1, 0], rec.points["K"][0, 1], rec.points["K"][-1, 1]))
    say("gating variables there: n %.4f  m %.4f  h %.4f" % tuple(rec.membrane[q][k, 0] for q in ("n", "m", "h")))
    amap = rec.membrane_map
    fired = ~np.isnan(amap["activation_time"])
    say("membrane map: %d of %d facets crossed 0 mV%s" % (fired.sum(), len(fired), "" if not fired.any() else
        ", first at t = %.3f ms, last at %.3f ms" % (1.0e3 * np.nanmin(amap["activation_time"]), 1.0e3 * np.nanmax(amap["activation_time"]))))
    say("conduction velocity between the boxes (%d and %d facets): %.3f m/s from the map, %.3f m/s from the set means"
        % (len(rec.set_facets[1]), len(rec.set_facets[0]), rec.conduction_velocity(1, 0), rec.conduction_velocity(1, 0, method="set_mean")))
    busy = S.emi_solve_timer + S.knp_solve_timer + S.emi_ass_timer + S.knp_ass_timer + S.ode_solve_timer
    say("EMI iterations %.2f per step, KNP %.2f, %.2f ms per step (solve, assembly and ODE timers); timeseries written to "
        "results/data/3D/timeseries.h5" % (np.mean(S.emi_niter), np.mean([max(n) for n in S.knp_niter]), 1.0e3 * busy / len(rec.t)))
