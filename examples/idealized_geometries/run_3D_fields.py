#!/usr/bin/python3
"""A short run_3D.py configuration that shows the volume fields on the mesh itself: one axon is stimulated and phi and [K+] are sampled
on the device while the run goes on, once on the extracellular space alone and once on every cell (reference:
examples/idealized-geometries/make_figures_3D.py rebuilds such pictures from results.h5 with FEniCS).

    python run_3D_fields.py [resolution] [Tstop] [every]

Writes results/data/3D_fields/ecs.h5 and all.h5 -- /mesh/{points, connectivity, cells, tag, node_entity, node_tag} is the tetrahedral
mesh with one node per (vertex, subdomain), /<field>/vector_<k> holds one value per node and frame -- and ecs.xdmf / all.xdmf, which
ParaView opens: colour all.xdmf by phi and clip it to see the jump across the membranes, threshold by `tag` to tell ECS from ICS,
colour ecs.xdmf by c_K to watch potassium pile up around the stimulated axon."""
import sys

from idealized_common import make_solver, solver_parameters, Constant

OUT = "results/data/3D_fields/"
FIELDS = ("phi", "c_K")

if __name__ == "__main__":
    resolution = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    Tstop = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0e-3
    every = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    S = make_solver(dim=3, resolution=resolution, verbose=False)       # mm_hh (stimulated) on tag 1, mm_hh_no_stim on tag 2
    ecs = S.record_fields(fields=FIELDS, tags=(0,), every=every, name="ecs")
    every_cell = S.record_fields(fields=FIELDS, every=every, name="all")
    t = Constant(0.0)
    S.solve_system_active(Tstop, t, solver_parameters(3, resolution), filename=OUT)
    frame = every_cell.sample()
    inside = every_cell.node_tag != 0
    print("%d nodes for %d cells (%d in the ECS alone); at t = %.2f ms phi lies between %.1f and %.1f mV inside the axons, %.2f and "
          "%.2f mV outside" % (len(inside), len(every_cell.cells), len(ecs.node_tag), 1e3 * float(t), 1e3 * frame["phi"][inside].min(),
                               1e3 * frame["phi"][inside].max(), 1e3 * frame["phi"][~inside].min(), 1e3 * frame["phi"][~inside].max()))
    tm = every_cell.timing()
    print("%.1f us per frame of %d fields on the device (+ %.1f us copy), %.2f MB per frame against %.2f MB of fp64 DG vectors"
          % (1e3 * tm["sample_ms"], len(FIELDS), 1e3 * tm["copy_ms"], 1e-6 * 4 * len(FIELDS) * len(inside),
             1e-6 * 8 * len(FIELDS) * every_cell.connectivity.size))
    print("frames every %d steps in %secs.h5 and %sall.h5; open the .xdmf files in ParaView" % (every, OUT, OUT))
