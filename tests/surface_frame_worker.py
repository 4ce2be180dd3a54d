"""The child process of tests/test_gpu_surface.py::test_no_reorder_gives_the_same_bits: with the environment it is started in
(KNP_NO_REORDER=1) it builds the context of every case of surface_cases.CASES, samples every field and state plane once and writes
the frames to an .npz, together with whether the context kept the caller's cell order.
usage: surface_frame_worker.py out.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import surface_cases as SC                                                                           # noqa: E402

out = {}
for name, p in SC.CASES:
    dev, pb, s, models, tables, E = SC.device_case(name, p)
    try:
        out["%s_p%d_identity" % (name, p)] = int(np.array_equal(dev.cell_order, np.arange(pb.mesh.num_cells())))
        out["%s_p%d" % (name, p)] = SC.device_frame(dev, pb, s, models, SC.all_fields(pb), SC.state_names(name))[1]
    finally:
        dev.close()
np.savez(sys.argv[1], **out)
