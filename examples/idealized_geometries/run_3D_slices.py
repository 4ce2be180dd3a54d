#!/usr/bin/python3
"""A short run_3D.py configuration whose pictures are sampled on the device while it runs, instead of being rebuilt afterwards from
per-step field output (reference: examples/idealized-geometries/make_figures_3D.py evaluates the saved functions with FEniCS): one
x-y mid-plane image of phi and the ions, and one coarse volume of the extracellular potassium around the axons.

    python run_3D_slices.py [resolution] [Tstop] [every]

Writes results/data/3D_slices/{midplane,ecs}.h5 -- /<field>/vector_<n> are dense [nz, ny, nx] arrays, NaN where the grid has no
cell (the ECS-only volume is NaN inside the axons) -- and the XDMF sidecars midplane.xdmf / ecs.xdmf, which ParaView opens."""
import sys

import numpy as np

from idealized_common import make_solver, solver_parameters, Constant

OUT = "results/data/3D_slices/"

if __name__ == "__main__":
    resolution = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    Tstop = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0e-3
    every = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    S = make_solver(dim=3, resolution=resolution, verbose=False)
    lo, hi = S.mesh.coords.min(axis=0), S.mesh.coords.max(axis=0)
    z_mid = 0.5 * (lo[2] + hi[2])
    # a slice is a grid with one point along an axis; tags=(0,) keeps the extracellular cells only
    plane = S.record_grid((lo[0], lo[1], z_mid), (hi[0], hi[1], z_mid), (257, 33, 1), fields=("phi", "K", "Na", "Cl"), every=every,
                          name="midplane")
    ecs = S.record_grid(lo, hi, (65, 17, 17), fields=("K",), every=every, tags=(0,), dtype=np.float32, name="ecs")
    t = Constant(0.0)
    S.solve_system_active(Tstop, t, solver_parameters(3, resolution), filename=OUT)
    phi = plane.sample()["phi"][0]
    print("mid-plane %d x %d: phi between %.3f and %.3f mV at t = %.2f ms; %d of %d points of the volume are extracellular"
          % (phi.shape[1], phi.shape[0], 1e3 * np.nanmin(phi), 1e3 * np.nanmax(phi), 1e3 * float(t), (ecs.cells >= 0).sum(), ecs.cells.size))
    tm = plane.timing()
    print("locate %.3f ms, weights %.3f ms once; %.1f us per frame on the device (+ %.1f us copy)"
          % (tm["locate_ms"], tm["weights_ms"], 1e3 * tm["sample_ms"], 1e3 * tm["copy_ms"]))
    print("frames every %d steps in %smidplane.h5 and %secs.h5; open %smidplane.xdmf / %secs.xdmf in ParaView" % (every, OUT, OUT, OUT, OUT))
