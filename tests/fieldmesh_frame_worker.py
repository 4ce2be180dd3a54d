"""The child process of tests/test_gpu_fieldmesh.py::test_no_reorder_gives_the_same_bits: with the environment it is started in
(KNP_NO_REORDER=1) it builds the context of every case of fieldmesh_cases.CASES, samples every field once, continuous and not, and
writes the frames to an .npz together with what identifies their nodes -- (entity, tag), resp. (cell, dof) -- and whether the context
kept the caller's cell order.
usage: fieldmesh_frame_worker.py out.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "knp-emi-dg_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import fieldmesh_cases as FC                                                                         # noqa: E402

out = {}
for name, p in FC.CASES:
    sel = "ecs" if name == "2d" else "all"
    dev, pb = FC.device_case(name, p)
    try:
        out["%s_p%d_identity" % (name, p)] = int(np.array_equal(dev.cell_order, np.arange(pb.mesh.num_cells())))
        for cont in (True, False):
            s = FC.make_spec(name, p, sel, cont, cell_rank=dev.cell_rank)
            h, frame = FC.device_frame(dev, pb, s)
            dev.fieldmesh_destroy(h)
            key = "%s_p%d_%d" % (name, p, cont)
            out[key] = np.stack([frame[q] for q in FC.field_names(pb)])
            out[key + "_a"], out[key + "_b"] = (s.node_entity, s.node_tag) if cont else (s.cell, s.dof)
    finally:
        dev.close()
np.savez(sys.argv[1], **out)
