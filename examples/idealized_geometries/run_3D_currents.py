#!/usr/bin/python3
"""The stimulated run_3D.py configuration with what the model says about transport sampled on the device while it runs: an x-y
mid-plane slice of phi, the electric field -grad phi, the potassium flux J_K = -D_K grad K - z_K D_K psi K grad phi with its
diffusive share, and the current density F sum_k z_k J_k (current-source-density pictures, the diffusive and drift shares of K+
clearance).  Each is evaluated in the cell that owns the point: DG gradients are one-sided, so no finite differences across facets
or the membrane are involved.

    python run_3D_currents.py [resolution] [Tstop] [every]

Writes results/data/3D_currents/currents.h5 -- /phi/vector_<n> is a dense [1, ny, nx] array, the vector quantities are
[1, ny, nx, 3], NaN where the grid has no cell -- and currents.xdmf, which declares them as Vector attributes for ParaView."""
import sys

import numpy as np

from idealized_common import make_solver, solver_parameters, Constant

OUT = "results/data/3D_currents/"
FIELDS = ("phi", "efield", "flux_K", "diffusive_flux_K", "current")

if __name__ == "__main__":
    resolution = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    Tstop = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0e-3
    every = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    S = make_solver(dim=3, resolution=resolution, verbose=False)
    lo, hi = S.mesh.coords.min(axis=0), S.mesh.coords.max(axis=0)
    z_mid = 0.5 * (lo[2] + hi[2])
    plane = S.record_grid((lo[0], lo[1], z_mid), (hi[0], hi[1], z_mid), (257, 33, 1), fields=FIELDS, every=every, name="currents")
    t = Constant(0.0)
    S.solve_system_active(Tstop, t, solver_parameters(3, resolution), filename=OUT)
    frame = plane.sample()
    E, J, Jd, I = (frame[f][0] for f in FIELDS[1:])                  # [ny, nx, 3] each
    norm = lambda v: np.sqrt((v * v).sum(axis=-1))
    print("mid-plane %d x %d at t = %.2f ms: |E| up to %.3g V/m, |J_K| up to %.3g mol/(m^2 s) (diffusive share up to %.3g), "
          "|I| up to %.3g A/m^2" % (E.shape[1], E.shape[0], 1e3 * float(t), np.nanmax(norm(E)), np.nanmax(norm(J)), np.nanmax(norm(Jd)),
                                  np.nanmax(norm(I))))
    tm = plane.timing()
    print("locate %.3f ms, weights %.3f ms once; %.1f us per frame on the device (+ %.1f us copy)"
          % (tm["locate_ms"], tm["weights_ms"], 1e3 * tm["sample_ms"], 1e3 * tm["copy_ms"]))
    print("frames every %d steps in %scurrents.h5; open %scurrents.xdmf in ParaView" % (every, OUT, OUT))
