#!/usr/bin/python3
"""run_3D.py in two halves: run half of the steps and checkpoint, continue from the file in a second invocation, and compare with a
straight run.

    python run_3D_resume.py first  [resolution] [Tstop]    half of the steps, writes results/data/3D_resume/checkpoint.h5
    python run_3D_resume.py second [resolution] [Tstop]    a new process: resumes, finishes, stores the final state
    python run_3D_resume.py check  [resolution] [Tstop]    the straight run; prints the largest difference to the resumed one
    python run_3D_resume.py                                all three, each in a process of its own

With the default preconditioner the EMI hierarchy of the second half is rebuilt from the restored state, so the two runs agree
within the solver tolerances (relative differences around 1e-7 in the concentrations); with KNP_NO_AMG=1 they agree bit for bit and
the script prints 0."""
import os
import subprocess
import sys

import numpy as np

from idealized_common import make_solver, solver_parameters, Constant

OUT = "results/data/3D_resume/"


def fields(S):
    return {"c": S.c.array(), "c_elim": S.ion_list[-1]['c'].array(), "phi": S.phi.array(), "phi_M": S.phi_M_prev_PDE.array()}


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    resolution = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    Tstop = float(sys.argv[3]) if len(sys.argv) > 3 else 2.0e-3
    if what == "all":
        for part in ("first", "second", "check"):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), part, str(resolution), str(Tstop)])
        sys.exit(0)
    S = make_solver(dim=3, resolution=resolution)
    sp = solver_parameters(3, resolution)
    n = int(round(Tstop / float(S.dt)))
    half = max(n // 2, 1)
    t = Constant(0.0)
    if what == "first":
        S.solve_system_active(half * float(S.dt), t, sp, filename=OUT, checkpoint_every=half)
        print("checkpoint after step %d at t = %g: %scheckpoint.h5" % (half, float(t), OUT))
    elif what == "second":
        S.solve_system_active(Tstop, t, sp, filename=OUT, resume=OUT + "checkpoint.h5")
        np.savez(OUT + "resumed.npz", **fields(S))
        print("resumed at step %d, finished %d steps at t = %g" % (half, n, float(t)))
    elif what == "check":
        S.solve_system_active(Tstop, t, sp, filename=OUT + "straight/")
        got = np.load(OUT + "resumed.npz")
        worst = 0.0
        for name, a in fields(S).items():
            d = float(np.abs(a - got[name]).max() / np.abs(a).max())
            worst = max(worst, d)
            print("  %-7s largest difference %.3e of its maximum" % (name, d))
        print("largest difference between the resumed and the straight run: %.3e" % worst)
    else:
        sys.exit("usage: run_3D_resume.py [first|second|check] [resolution] [Tstop]")
