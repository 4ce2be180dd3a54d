#!/usr/bin/python3
"""A short run_3D.py configuration that shows what happens ON the membrane: one axon is stimulated and the membrane potential, the
potassium channel current, the extracellular potassium at the membrane and the gating variable n are sampled per membrane facet on
the device while the run goes on (reference: examples/idealized-geometries/make_figures_3D.py and
examples/rat-neuron/make_figures_rat_neuron.py rebuild such pictures from results.h5 with FEniCS).

    python run_3D_membrane.py [resolution] [Tstop] [every]

Writes results/data/3D_membrane/membrane.h5 -- /surface/{points, connectivity, facet, tag, cells, area} is the triangle mesh of
the membrane, /<plane>/vector_<k> holds one value per triangle and frame -- and membrane.xdmf, which ParaView opens: colour the
surface by phi_M and play the frames to watch the action potential travel along the stimulated axon (tag 1)."""
import sys

import numpy as np

from idealized_common import make_solver, solver_parameters, Constant

OUT = "results/data/3D_membrane/"
PLANES = ("phi_M", "I_ch_K", "c_K_e", "I_ch_total")

if __name__ == "__main__":
    resolution = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    Tstop = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0e-3
    every = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    S = make_solver(dim=3, resolution=resolution, verbose=False)       # mm_hh (stimulated) on tag 1, mm_hh_no_stim on tag 2
    m = S.record_membrane(fields=PLANES, states=("n",), every=every)
    t = Constant(0.0)
    S.solve_system_active(Tstop, t, solver_parameters(3, resolution), filename=OUT)
    frame = m.sample()
    stimulated = S.surfaces.array()[m.facets] == 1
    print("%d membrane facets (%d on the stimulated axon); at t = %.2f ms phi_M lies between %.1f and %.1f mV there, %.1f and %.1f mV "
          "on the others" % (len(m.facets), stimulated.sum(), 1e3 * float(t), 1e3 * frame["phi_M"][stimulated].min(),
                             1e3 * frame["phi_M"][stimulated].max(), 1e3 * frame["phi_M"][~stimulated].min(),
                             1e3 * frame["phi_M"][~stimulated].max()))
    tm = m.timing()
    print("%.1f us per frame of %d planes on the device (+ %.1f us copy)" % (1e3 * tm["sample_ms"], len(m.planes), 1e3 * tm["copy_ms"]))
    print("frames every %d steps in %smembrane.h5; open %smembrane.xdmf in ParaView" % (every, OUT, OUT))
